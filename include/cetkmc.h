/*
 * cetkmc.h -- C ABI of the MI355X-native rejection-free KMC stepping engine
 *             (libcetkmc_hip.so; hand-written HIP kernels for gfx950).
 *
 * The reference (codebits1001/CET-driven-simulation-for-3D-printing-AM-KMC-Approach)
 * is pure Python and has no FFI layer: its boundary for this path is the plain Python
 * call surface of kmc_simulation.run_kmc / kmc_event_rates.get_event_rates /
 * thermal_solver.update_temperature*.  Each entry point below names the reference
 * code it replaces (file:line relative to the reference root).  The Python modules of
 * the same names in this repository bind these symbols with ctypes.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; cetkmc_last_error()
 *     returns a thread-local message.  Nothing throws across the boundary.
 *   - the caller owns all host buffers; the library owns all device memory behind the
 *     opaque handle.  A handle is not thread-safe; use one handle per host thread.
 *   - host arrays are C-contiguous (L,L,L), axis 0 (i) slowest -- the reference layout.
 *   - there is NO CPU fallback: without a usable gfx950 device cetkmc_create fails.
 */
#ifndef CETKMC_H
#define CETKMC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CETKMC_ABI_VERSION 1

/* Model constants (defaults = reference constants.py:34-148, thermal_solver.py:6-9).
 * Passed by the host so that derived values carry the host's IEEE rounding. */
typedef struct cetkmc_params {
    double nu;             /* constants.py:70  NU            */
    double nu_dep;         /* constants.py:71  NU_DEP        */
    double E_b[3];         /* constants.py:74,80,84  W,Re,C  */
    double E_diff[3];      /* constants.py:75,81,85          */
    double kT;             /* constants.py:63  K_T           */
    double T_melt;         /* constants.py:64                */
    double I0;             /* constants.py:129               */
    double delta_T_c;      /* constants.py:123               */
    double K_nuc;          /* constants.py:130               */
    double beta_imp_nuc;   /* constants.py:131               */
    double max_imp_frac;   /* constants.py:90                */
    double rate_threshold; /* constants.py:145               */
    double anisotropy;     /* constants.py:102               */
    double impurity_re;    /* constants.py:82                */
    double impurity_c;     /* run_kmc / get_event_rates argument */
    double alpha;          /* thermal_solver.py:9   K/(RHO*CP)   */
    double inv_dx2;        /* thermal_solver.py:79,114  1/dx^2   */
    double T_clip_lo;      /* thermal_solver.py:105,117  T_SUB   */
    double T_clip_hi;      /* thermal_solver.py:105,117  1.1*T_MELT */
    double T_nan;          /* kmc_simulation.py:249  nan_to_num(nan=T_SUB) */
    double rho_cp;         /* thermal_solver.py:102  RHO*CP      */
    double latent_coef;    /* thermal_solver.py:102  200e3/CP    */
} cetkmc_params;

/* One KMC event (an element of the list get_event_rates returns,
 * kmc_event_rates.py:72,109,132,158).  64 bytes. */
typedef struct cetkmc_event {
    int32_t type;       /* 0 'dep', 1 'diff', 2 'nuc', 3 'att'; -1 = none            */
    int32_t pos[3];     /* (i,j,k) of the event site                                   */
    int32_t target[3];  /* diff: destination, att: source neighbour, else (-1,-1,-1)   */
    int32_t atom;       /* species the event writes (dep: 0 until the species is drawn)*/
    double  rate;       /* [1/s]                                                       */
    int64_t dep_rank;   /* dep: index among the deposition candidates in row-major
                           (j,k) order (selects the reference's per-candidate species
                           draw, kmc_event_rates.py:65); else -1                       */
    double  theta;      /* orientation written to the updated site (set by apply)     */
    double  phi;
} cetkmc_event;

enum { CETKMC_DEP = 0, CETKMC_DIFF = 1, CETKMC_NUC = 2, CETKMC_ATT = 3 };

/* Result of one full-lattice rate sweep (kmc_simulation.py:253-259). */
typedef struct cetkmc_sweep_info {
    double  total;      /* canonical-tree sum of all event rates           */
    int64_t n_events;   /* len(events)                                                 */
    int64_t n_dep;      /* number of deposition candidates (= RNG draws of the sweep)  */
} cetkmc_sweep_info;

/* Arguments of the batched stepping loop (kmc_simulation.py:246-332, n iterations).
 * All pointers are HOST pointers; arrays are copied to the device once per call -- or ahead of the call by
 * cetkmc_stage_inputs(), after which cetkmc_run_steps() takes the SAME arguments with all four input pointers NULL. */
typedef struct cetkmc_run_args {
    int64_t step0;            /* global index of the first step (thermal cadence step%20) */
    int64_t n_steps;
    double  defect_fraction;  /* kmc_simulation.py:323                                  */
    const double* u_pick;     /* [n] random.random() for r            (:265)            */
    const double* u_defect;   /* [n] random.random() defect draws (:323) or NULL if defect_fraction==0 */
    const double* u_np;       /* NumPy global stream, consumed in order                 */
    int64_t np_cap;           /* number of doubles in u_np                              */
    int32_t rng_mode;         /* 0: reference stream (n_dep species draws per step + 2 orientation
                                    draws per dep/nuc event);
                                 1: counter-based species draw, stream holds only the orientation draws;
                                 2: every uniform counter based -- u(seed, step, key), the keys of Mode B's box 0 (pick
                                    1<<40, theta 2<<40, phi 3<<40, defect 4<<40, species j*L+k): u_pick / u_defect / u_np
                                    are not read and may be NULL.  This is what cetkmc_run_supersteps(box == L) runs */
    uint64_t seed;            /* rng_mode 1 key                                         */
    int32_t thermal_mode;     /* 0 none, 1 update_temperature_cet every 20 steps (:248-250),
                                 2 update_temperature (laser) every 20 steps             */
    double  thermal_dt;       /* dt of the thermal update (run_kmc uses 1e-6)           */
    const double* q_planes;   /* thermal_mode 2: [n_q][L*L] source planes, consumed in order.
                                 Continuing a batch that stopped with status 2 ON an update step (step0 + steps_done a
                                 multiple of 20; that step's update is already in the field, cetkmc_run_result.status):
                                 the continuation starts at the same step0 = that step and supplies that step's plane
                                 again as q_planes[0].  It is not read a second time, but it is counted again in q_used.
                                 The handle remembers the applied update only until the next upload (of any field, a
                                 defects-only one included) or direct temperature update (cetkmc_thermal_cet, _thermal_laser,
                                 the updates of cetkmc_time_thermal): after either, a call starting at that step applies
                                 the update like any other (CETKMC_CACHE_APPLIED).  Everything else leaves the marker --
                                 cetkmc_remelt, cetkmc_set_remelt, cetkmc_set_thermal_substeps, cetkmc_set_thermal_scheme, cetkmc_set_params,
                                 cetkmc_time_sweeps, the read-only calls: behind them the continuation still skips that
                                 step's update (and its melt pass, whatever the switches say by then) */
    int64_t n_q;
    int32_t use_latent;       /* thermal_mode 2: latent-heat term on/off                */
    int32_t profile;          /* 1: time every rate-sweep launch with hipEvents; 3: every 8th launch, every 4th in batches of <= 64
                                 steps (an event pair costs ~4 us of stream time); 2: time every phase (cetkmc_get_counters) */
    int32_t incremental;      /* 0: every step evaluates the whole lattice (get_event_rates, kmc_event_rates.py:162);
                                 1: exact incremental mode -- between temperature updates only the rows whose
                                    rates the previous event can have changed are re-evaluated (identical
                                    results: the canonical summation tree is rebuilt from the same row sums) */
} cetkmc_run_args;

typedef struct cetkmc_run_result {
    int64_t steps_done;
    int32_t status;           /* 0 ok, 1 terminated (no valid events, :260-262), 2 u_np exhausted: continue with a call
                                 whose step0 is this call's step0 + steps_done and whose u_np starts at np_used.  When
                                 that step is a temperature-update step its update has been applied already and the
                                 continuation does not repeat it (cetkmc_run_args.q_planes says what it must supply, and
                                 which calls in between make the handle forget the applied update) */
    int64_t np_used;          /* doubles of u_np consumed                               */
    int64_t q_used;           /* thermal_mode 2: source planes consumed by the executed steps (and by the step a batch
                                 stopped in: its update precedes the selection); planes queued behind an early stop
                                 are not counted, their updates pass through */
    int64_t nucleation_count; /* running total on the handle (:310)                     */
    double  sweep_ms_total;   /* profile: sum of rate-sweep kernel durations            */
    int64_t sweep_launches;
    double  wall_ms;          /* device time of the whole call (hipEvents on the stream) */
    int64_t full_sweeps;      /* steps that evaluated the whole lattice (= steps issued unless incremental) */
    double  min_margin;       /* selection margin of the batch: min over its steps of the distance of r = u * total from the
                                 nearer end of the chosen event's interval of the cumulative sum, divided by the total
                                 (this rank's picks; 1.0 if it made none).  The canonical tree sum and the reference's
                                 sequential sum (kmc_simulation.py:259,265-274) differ by <= ~1e-13 relative: a margin
                                 below that means the reference's scan could have stopped at the neighbouring event. */
} cetkmc_run_result;

/* Mode B -- synchronous super-steps (NOT in the reference; SURVEY.md section 8(f)4, DESIGN.md "Mode B").
 * The lattice is tiled by (L/box)^3 cubic boxes; every super-step runs the ordinary full rate sweep and then
 * every box executes at most one event picked from its active octant (octant = step % 8), so several thousand
 * events are executed per sweep.  box: even, 8..16, divides L -- or box == L: ONE domain without octants, which is
 * exactly a Mode A step (kmc_simulation.py:253-327) driven by the counter uniforms of box 0 (single process).
 * All uniforms are counter based (seed, step, key).
 * null_events: with R_max = the largest window total of the super-step, box d executes its pick only with probability
 * R_d / R_max (else a null event, logged as type -2): every event of an active window then fires with probability
 * rate / R_max per visit -- proportional to its rate everywhere, like the reference's global pick
 * (kmc_simulation.py:265-274).  0: every non-idle box executes its pick (boxes with few events are over-sampled).
 * The trajectory is not the reference's; its bit-exact comparator is the oracle's orc_run_supersteps. */
typedef struct cetkmc_super_args {
    int64_t step0;            /* global index of the first super-step (thermal cadence step%20, octant step%8) */
    int64_t n_steps;
    int32_t box;
    double  defect_fraction;
    uint64_t seed;
    int32_t thermal_mode;     /* as cetkmc_run_args */
    double  thermal_dt;
    const double* q_planes;
    int64_t n_q;
    int32_t use_latent;
    int32_t null_events;      /* see above */
} cetkmc_super_args;

/* Work issued, bytes moved and (while cetkmc_run_args.profile == 2) device time per phase, accumulated on the
 * handle since creation / the last reset.  Algorithmic bytes: 9 B per owned voxel per rate sweep (class u8 + rate
 * table f64; the recompute variant streams T f64 instead), 16 B per owned voxel per temperature update and 16 B per
 * owned voxel per rate-table refresh (T read, entry written). */
typedef struct cetkmc_counters {
    int64_t steps;              /* batched Mode A steps executed (cetkmc_run_steps)               */
    int64_t sweeps;             /* full rate sweeps launched (any entry point)                     */
    int64_t incremental_steps;  /* steps that re-evaluated dirty rows only                         */
    int64_t thermal_updates;
    int64_t supersteps;         /* Mode B super-steps executed                                     */
    int64_t bytes_h2d, bytes_d2h;               /* host <-> device bytes moved by this handle       */
    int64_t alg_bytes_sweep, alg_bytes_thermal; /* algorithmic bytes of the work issued             */
    int64_t profiled_steps;     /* steps the ms_* fields below cover                               */
    double  ms_thermal, ms_interface /* rate table + interface list kernels */, ms_sweep, ms_dirty_rows, ms_reduce, ms_select_apply;
    int64_t alg_bytes_table;    /* rate-table refreshes (k_rate_table)                             */
    int64_t table_updates;      /* rate-table refreshes launched                                   */
    int64_t interface_launches; /* full interface-list evaluations launched                        */
    double  ms_comm;            /* profile 2, multi-rank handles: device time between the hipEvent pairs around every
                                   collective of the profiled steps (block-sum / event all-gathers, temperature-halo and
                                   boundary-layer exchanges); part of ms_reduce / ms_select_apply / ms_thermal above   */
    int64_t comm_calls;         /* collectives those pairs bracketed                               */
    int64_t deferred_steps;     /* cetkmc_run_steps: steps launched as a selection alone, their event applied inside the next
                                   rate-sweep launch (option apply_in_sweep); counts launches issued, so a batch that stops
                                   early still counts every deferred step the host queued                           */
    int64_t early_tiles;        /* tiles of the next step's sweep that those steps' selection launches ran (option
                                   early_tiles); launches issued, as above                                             */
} cetkmc_counters;

const char* cetkmc_last_error(void);
int cetkmc_abi_version(void);
/* hash of the sources the library was compiled from (-DCETKMC_SRC_HASH, set by cetkmc/_lib.build_library; "unknown" for a
 * hand build): the binding compares it with the sources beside it and rebuilds / refuses a stale library */
const char* cetkmc_source_hash(void);
/* sizeof of an ABI struct by name ("params", "event", "sweep_info", "run_args", "run_result", "super_args", "counters",
 * "host_comm", "ens_args", "ens_analysis", "front_stats", "layer_rec", "texture_args", "grain_rec",
 * "solid_info", "solid_args", "solid_rec", "origin_rec", "local_args", "remelt_info", "substep_info", "implicit_info",
 * "thermal_boundary", "boundary_info", "beam", "beam_info", "shift", "shift_info"); -1 for an unknown name.  Lets a binding check its mirrors against the library it loaded. */
int cetkmc_struct_size(const char* name);
/* 1 when the sums of row (plane i + di, row j + dj) depend on voxel (i, j, k), else 0: the rule the incremental mode's dirty
 * list and the stale rows of a deferred event are built from (at most 11 offsets, all within [-2, 2]^2).  Host function; needs no
 * device. */
int cetkmc_dirty_offset(int di, int dj);
/* The stale rows of a deferred step's pending event -- type (cetkmc_event::type, < 0: none), pos[0..1] and, for a diffusion,
 * target[0..1]: the rows the sweep launch that applies the event leaves to its apply block.  cetkmc_stale_row: 1 when row j
 * of global plane gi is one (a function of the record alone; lattice bounds are the caller's), else 0.  cetkmc_stale_rows:
 * the apply block's own enumeration for an L^3 lattice, (plane, row) pairs into rows[22][2]; returns their number (never more
 * than 22; entries beyond 22 would not be written).  Host functions; need no device. */
int cetkmc_stale_row(int type, const int pos[2], const int target[2], int gi, int j);
int cetkmc_stale_rows(int type, const int pos[2], const int target[2], int L, int rows[][2]);
/* The tile of the census-free streaming launches (option fused_tiles) that owns row j of plane gi of a one-slab lattice with
 * 128 < L <= 256: tiles own consecutive ranges of items, item = gi * ((L + 1) / 2) + j / 2, a pair of rows.  -1 outside that
 * shape or the lattice.  Host function; needs no device. */
int cetkmc_table_tile_of(int L, int gi, int j);
/* Which launch stores row j of plane gi under option early_tiles = early_tiles, unless the pending event makes the row stale:
 * 1 = a tile of the deferred step's selection launch (cetkmc_table_tile_of() < early_tiles), 0 = a tile of the sweep launch
 * behind it, -1 where cetkmc_table_tile_of() is.  Host function; needs no device. */
int cetkmc_early_tile_row(int L, int early_tiles, int gi, int j);
/* 1 when the census-free tiles (option table_lane_skip) load the 8 rate-table entries of the lane whose 8 class bytes are
 * class8 (byte h = voxel k0 + h, little endian): some byte is empty (bit 0) or holds a non-zero count (bits 7:2).  0: all
 * bytes are 0x00 or 0x02, the row reduction masks every entry of the lane.  Host function; needs no device. */
int cetkmc_lane_needs_values(uint64_t class8);
/* What a lane of those tiles requests under option lane_sums while the lane table is fresh, from its 8 class bytes and the
 * count byte of its chunk (0..8 = the non-zero entries the last building sweep saw, 0xFF = poisoned): CETKMC_LANE_REQ_SUM,
 * the 8 B lane sum, where every class byte is 0x01 and the count byte is a count; else CETKMC_LANE_REQ_VALUES, the 64 B of
 * entries, where cetkmc_lane_needs_values() holds; else CETKMC_LANE_REQ_NONE.  Host function; needs no device. */
enum cetkmc_lane_req { CETKMC_LANE_REQ_NONE = 0, CETKMC_LANE_REQ_VALUES = 1, CETKMC_LANE_REQ_SUM = 2 };
int cetkmc_lane_request(uint64_t class8, int count_byte);
/* Inspection of a handle's lane table (tests; one small kernel and a synchronisation): fresh = 1 when the deferred launches
 * would read lane sums now; chunks = owned chunks of 8 table entries (0: the shape has no lane table), of which `usable` hold a
 * count and `poisoned` 0xFF; builds = plain sweep launches that have built the table so far; builds_thermal = temperature
 * updates whose tiles built it (option lane_build). */
typedef struct cetkmc_lane_table_info { int64_t fresh, chunks, usable, poisoned, builds, builds_thermal; } cetkmc_lane_table_info;
int cetkmc_lane_table(void* handle, cetkmc_lane_table_info* out);
/* The owned chunks of the lane table as they stand (tests; two copies and a synchronisation): n = cetkmc_lane_table()'s
 * `chunks` sums and count bytes, chunk (plane, row, k / 8) at (plane * L + row) * (row pitch / 8) + k / 8. */
int cetkmc_lane_table_copy(void* handle, double* sums, uint8_t* counts, int64_t n);
/* The node and the non-zero count of a chunk's 8 entries as the temperature tiles that build the lane table form them, in
 * `lane` (0..3) of the four lanes that hold the chunk: lane l has x8[2l] + x8[2l+1], adds the pair sum of lane l ^ 1, then the
 * quad sum of lane l ^ 2.  cetkmc_tree8: the row reduction's expression ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)) of the same
 * entries.  Host functions; need no device. */
void cetkmc_lane_quad_node(const double* x8, int lane, double* sum, int* count);
double cetkmc_tree8(const double* x8);
/* What a handle keeps between calls, as bits of cetkmc_invalidates()'s result. */
enum cetkmc_cache {
    CETKMC_CACHE_SWEEP = 1,     /* row and block sums of the last rate sweep (cetkmc_select, cetkmc_row_sums read them) */
    CETKMC_CACHE_TABLE = 2,     /* per-voxel rate table of the current temperature field and parameters */
    CETKMC_CACHE_IFC = 4,       /* the listed (interface) voxels' sums and event counts */
    CETKMC_CACHE_APPLIED = 8,   /* the temperature update a batch stopped with status 2 has already applied */
    CETKMC_CACHE_STAGED = 16    /* a batch staged by cetkmc_stage_inputs */
};
/* The caches a named cause makes stale, as a mask of cetkmc_cache bits; -1 for an unknown name.  It reads the table every
 * mutating entry point of the library invalidates by; the names are that table's (DESIGN.md section 20 lists them).  Host
 * function; needs no device. */
int cetkmc_invalidates(const char* cause);
int cetkmc_device_count(int* n);

/* Lifetime.  n_slabs > 1 with all device_ids equal splits the lattice into axis-0 slabs
 * inside one process on one GPU (decomposition check mode).  Multi-GPU runs use one
 * process per GPU: cetkmc_create_rank + an RCCL unique id shared by the launcher. */
int cetkmc_create(const cetkmc_params* p, int L, int n_slabs, const int* device_ids, void** handle);
int cetkmc_get_unique_id(char out[128]);
int cetkmc_create_rank(const cetkmc_params* p, int L, int rank, int nranks, int device_id,
                       const char unique_id[128], void** handle);
/* Bring-up / test transport: the same per-rank device code path as cetkmc_create_rank, with the three collectives
 * relayed through host callbacks (e.g. torch.distributed over gloo) instead of RCCL; the call synchronises the
 * stream around every exchange, and several ranks may share one GPU.  Callbacks return 0 on success.
 *   allgather(user, send, recv, nbytes): every rank contributes nbytes at `send`; recv gets nranks*nbytes in rank order
 *   exchange (user, lo, hi, send_lo, recv_lo, send_hi, recv_hi, nbytes): swap nbytes with rank lo and with rank hi
 *                                                                       (-1: no such neighbour)                    */
typedef int (*cetkmc_allgather_fn)(void* user, const void* send, void* recv, int64_t nbytes);
typedef int (*cetkmc_exchange_fn)(void* user, int lo, int hi, const void* send_lo, void* recv_lo, const void* send_hi,
                                  void* recv_hi, int64_t nbytes);
typedef struct cetkmc_host_comm {
    cetkmc_allgather_fn allgather;
    cetkmc_exchange_fn exchange;
    void* user;
} cetkmc_host_comm;
int cetkmc_create_rank_host(const cetkmc_params* p, int L, int rank, int nranks, int device_id, const cetkmc_host_comm* hc,
                            void** handle);
int cetkmc_destroy(void* handle);
int cetkmc_set_params(void* handle, const cetkmc_params* p);
int cetkmc_sync(void* handle);
/* tuning / A-B switches: "sweep_variant" 0 = simple kernel, 1 = streaming kernel (LDS census) + per-voxel rate table (default),
 * 2 = streaming kernel that recomputes the nucleation rates in every sweep, 3 = census-free table sweep (class bytes + rate table
 * streamed once, no LDS; same bits, measured no faster -- DESIGN.md section 13), 4 = the same with one block per plane and the block
 * sums folded in the sweep launch (no k_plane_reduce; faster at L <= 128 only -- which is why handles on which this option was
 * never set use it for L <= 128 and variant 1 above); "interface_every_step" 1 = evaluate the
 * whole interface list before every full sweep instead of only after a temperature update; "thermal_lookahead" 1 = the next
 * temperature update of a batch and its rate table are computed ahead on a second stream (single process; same bits;
 * default 0: measured slower); "thermal_table" 1 (default) = the default temperature tiles also write
 * the new field's rate table and deposition rates (no k_rate_table launch after an update; same bits), 0 = separate launch;
 * "thermal_variant" 0 = one thread per voxel, 1 = plane marching (default:
 * k_thermal_tiles16 -- 16 x 256 tiles, 1024 threads with 2 rows each, 16 planes per block -- where the tiles cover the lattice
 * exactly, else k_thermal_march), 2 = k_thermal_march everywhere, 3 = 16-row tiles with 4 rows per thread, 4 = the 8-row
 * k_thermal_tiles (round-2 kernel), 5 = 16 x 128 tiles (A/B variants);
 * "thermal_planes_per_block" (march / 8-row tiles), "thermal_planes_per_block16" (16-row tiles); "reserve_batch" n = allocate the
 * device buffers and hipEvents of a batch of n steps now (a bench keeps hipMalloc / hipEventCreate out of its timed region);
 * "apply_in_sweep" 1 (default) = cetkmc_run_steps applies the event of a step whose successor is no temperature-update step
 * (and is not the call's last) inside the next sweep launch (one process, one slab, sweep_variant 1, 128 < L <= 256, full
 * sweeps; same bits), 0 = every step's event applied by its own selection launch;
 * "fused_tiles" 1 (default) = the sweep launch that applies a pending event reduces its rows without the neighbour census, from
 * each voxel's own class byte and the rate table (no LDS ring, no barriers; one process, one slab, 128 < L <= 256; same bits),
 * 2 = the plain streaming launch at that shape as well, 0 = the ring tiles of sweep_variant 1 in both;
 * "table_lane_skip" 1 (default) = those census-free tiles request a lane's class bytes first and its rate-table entries only if
 * cetkmc_lane_needs_values() holds for them (same bits, fewer bytes), 0 = every lane's entries;
 * "lane_sums" 1 (default) = with table_lane_skip, a lane whose 8 voxels are empty and unlisted requests one stored sum (8 B, built
 * by the plain sweep that follows a table write, dropped per chunk wherever an entry is written: cetkmc_lane_request()) instead
 * of its 8 entries (same bits, fewer bytes; off while thermal_lookahead is on), 0 = entries;
 * "lane_build" 1 (default) = with lane_sums, the temperature tiles that write the rate table (thermal_table, L a multiple of 256)
 * store the lane table of the entries they write as well, so the plain sweep behind the update does not build it (same bits),
 * 0 = that sweep builds; "lane_sweep" 1 (default) = a plain sweep launch reads lane sums while the lane table is fresh, like the
 * deferred launches (same bits, fewer bytes), 0 = the plain launch reads every entry;
 * "early_tiles" E = the selection launch of a deferred step also runs the first E census-free tiles of the next step's sweep
 * (values past the tile count mean all of them), which the next sweep launch then leaves out; they store into the handle's
 * second pair of row-sum buffers, which becomes the current pair (same bits; DESIGN.md sections 13 and 20), 0 = the selection
 * block alone and one pair, -1 (default) = a quarter of the tiles (1024 of 4096 at 256^3, where it was measured);
 * "early_blocks" G (default 256, one per CU) = those E tiles run in G blocks, each taking every G-th tile in turn (0 or G >= E:
 * one block per tile); "poison_alt_rows" 1 (tests) = the pair such a step is about to write is filled with 0xFF bytes
 * first, so that a row no launch stores would show as NaN in the next total, 0 (default) = no fill */
int cetkmc_set_option(void* handle, const char* key, int64_t value);
/* planes [*i0,*i1) owned by this handle (whole lattice unless created with create_rank) */
int cetkmc_owned_planes(void* handle, int* i0, int* i1);

/* Lattice transfer in the reference's dtypes (run_kmc's arrays, kmc_simulation.py:226-233).
 * NULL pointers leave the field unchanged / are not written. */
int cetkmc_upload(void* handle, const int64_t* state, const double* theta, const double* phi,
                  const double* T, const int64_t* defects);
int cetkmc_download(void* handle, int64_t* state, double* theta, double* phi, double* T,
                    int64_t* defects);
/* Narrow transfer of planes [i_begin,i_end) only (arrays shaped (i_end-i_begin, L, L)); the
 * range must cover the owned planes plus the 2-plane halo (clipped to the lattice). */
int cetkmc_upload_planes(void* handle, int i_begin, int i_end, const uint8_t* state,
                         const double* theta, const double* phi, const double* T,
                         const uint8_t* defects);
int cetkmc_download_planes(void* handle, int i_begin, int i_end, uint8_t* state, double* theta,
                           double* phi, double* T, uint8_t* defects);
/* defects.track_defects result (defects.py:4-19), full lattice, 0/1 bytes */
int cetkmc_set_defects(void* handle, const uint8_t* mask);
/* latent-heat reference state (thermal_solver.py:98); NULL = snapshot the current state */
int cetkmc_set_prev_state(void* handle, const int64_t* prev_state);

/* thermal_solver.update_temperature_cet (thermal_solver.py:107-117); scrub_nan applies
 * np.nan_to_num(T, nan=T_SUB) first (kmc_simulation.py:249). */
int cetkmc_thermal_cet(void* handle, double dt, int scrub_nan);
/* thermal_solver.update_temperature (thermal_solver.py:36-105).  q_top = (L,L) volumetric
 * source of plane i=L-1, i.e. I_surface/VOXEL_SIZE built by the host as the reference does
 * (:82-95); the latent term uses the state set by cetkmc_set_prev_state. */
int cetkmc_thermal_laser(void* handle, double dt, const double* q_top, int use_latent, int scrub_nan);

/* kmc_event_rates.get_event_rates as a reduction (kmc_event_rates.py:162-176 +
 * kmc_simulation.py:259): evaluates every event rate, leaves row/block sums on the device. */
int cetkmc_rate_sweep(void* handle, cetkmc_sweep_info* info);
/* kmc_simulation.py:265-274: pick the event whose cumulative rate first reaches r
 * (canonical-tree order).  Needs a preceding cetkmc_rate_sweep. */
int cetkmc_select(void* handle, double r, cetkmc_event* out);
/* kmc_simulation.py:276-327: apply one event; theta/phi are the two np.random.uniform draws
 * (dep/nuc); make_defect is the outcome of the defect-injection draw (:323). */
int cetkmc_apply(void* handle, const cetkmc_event* ev, double theta_new, double phi_new, int make_defect);
/* kmc_event_rates.get_event_rates in list form (parity / small L).  *n receives len(events);
 * at most cap are written, in the reference's order. */
int cetkmc_enumerate_events(void* handle, cetkmc_event* buf, int64_t cap, int64_t* n);
/* Row sums/counts of the last sweep, shape (L,3,L) = [i][category dep/diff/empty][j]. */
int cetkmc_row_sums(void* handle, double* rowsum, int32_t* rowcnt);

/* kmc_simulation.py:246-332 for n steps without host round trips. totals/events/n_events
 * (each [n_steps], may be NULL) receive the per-step total rate, chosen event and len(events). */
int cetkmc_run_steps(void* handle, const cetkmc_run_args* args, cetkmc_run_result* res,
                     double* totals, cetkmc_event* events, int64_t* n_events);
/* Puts the host inputs of ONE coming batch (u_pick, u_defect, u_np, q_planes of `args`) into the handle's device
 * buffers and waits for the copies.  The next cetkmc_run_steps() call may then pass the same args with all four input
 * pointers NULL: it checks step0 / n_steps / np_cap / n_q / thermal_mode against the staged batch and copies nothing
 * (bench.py: inputs resident in HBM before the timed region).  Any other stepping call drops the staged batch, and so do
 * cetkmc_run_supersteps and cetkmc_set_option("reserve_batch") (they reuse or move the buffers); a second
 * cetkmc_stage_inputs replaces it.  The staged batch holds inputs only, nothing derived from the lattice: every other call
 * between the two -- uploads, cetkmc_set_params, the defect masks, cetkmc_set_prev_state, the direct temperature updates,
 * cetkmc_apply, the remaining options, the read-only calls -- leaves it valid, and the cetkmc_run_steps that consumes it
 * steps the lattice and parameters as they stand when IT is called (tests/test_gpu_live_handle_vs_oracle.py). */
int cetkmc_stage_inputs(void* handle, const cetkmc_run_args* args);

/* totals[n] (Mode A total of every super-step's sweep), events[n][D] or NULL (type -1: idle box, -2: null event),
 * n_executed[n] events applied per super-step, dt_event[n] (or NULL) the time increment PER EXECUTED EVENT of every
 * super-step: kmc_simulation.py:331-332 restated with the super-step's total and one counter uniform (key 6<<40),
 * dt_event[g] = max(-ln(max(1e-12, u_g)) / totals[g], 1e-12); simulated time advances by n_executed[g] * dt_event[g]
 * (n_executed summed over ranks; dt_event is the same on every rank).  res->np_used is 0.
 * Across ranks (cetkmc_create_rank*; needs (L / nranks) % box == 0): the boxes are sharded with the slabs -- D is the
 * number of THIS rank's boxes ((L / nranks / box) * (L / box)^2, global box order = rank order), events / n_executed /
 * res->nucleation_count cover this rank's boxes only (the caller sums them), totals are global.  Per super-step the
 * ranks exchange the block sums (all-gather, as Mode A) and the events of their boundary box layers (neighbour
 * send/recv, (L/box)^2 records each way): every rank applies its neighbours' boundary events to its own copy of the
 * halo planes and of the owned planes a diffusion target reached. */
int cetkmc_run_supersteps(void* handle, const cetkmc_super_args* a, cetkmc_run_result* res, double* totals,
                          cetkmc_event* events, int64_t* n_executed, double* dt_event);

/* Mode B with a local event loop (NOT in the reference): every box executes SEVERAL events per
 * super-step, up to a common time horizon (Shim & Amar's synchronous sublattice scheme), so the event mix stays
 * rate-proportional without idling the boxes.  box 8 only (windows of 4 x 4 x 4 voxels), L % 8 == 0.  Per super-step g:
 * temperature update, sweep, totals[g], dt_event[g] and every box's first pick exactly as cetkmc_run_supersteps; then
 * R_max = the largest window total of the non-idle boxes, horizon[g] = horizon_events / R_max (0 when every box is idle),
 * and box d runs: t = 0, m = 0; while it holds a pick: stop when m == max_events (the box counts in n_capped[g]); draw
 * u = u(seed, g, 7<<40 | m<<24 | d), w = -ln(u) / R with R the window total the pick was made from (u == 0: w = +inf);
 * stop when t + w > horizon[g] (with an infinite horizon that never holds, also for w = +inf: the event executes); else t += w, apply the pick (uniforms: theta 2<<40 | m<<24 | d, phi 3<<40 | m<<24 | d,
 * defect 4<<40 | m<<24 | d, deposition species m<<44 | j * L + k), ++m, and while m < max_events pick again from the same
 * window on the lattice as the box's own events left it (uniform 1<<40 | m<<24 | d; same leaves, window tree, descent and
 * slot scan as the first pick).  The windows' read ranges do not reach what another box writes, so the result is that of
 * the boxes running one after the other.  For m = 0 every key is cetkmc_run_supersteps'; with max_events = 1 and an
 * infinite horizon the call is cetkmc_run_supersteps(null_events = 0).
 * events[n][D][max_events] or NULL: the executed events of every box in order, unused slots as an idle box's record
 * (type -1); n_executed[n], dt_event[n] as above; horizon[n]; n_capped[n] boxes that executed max_events events.
 * Refused: box != 8 or L % 8 != 0, max_events outside 1..64, horizon_events <= 0 or NaN, thermal_mode 2, more than one
 * slab or a rank handle, an ensemble replica, sweep_variant < 1.  An origin map absorbs D * max_events records per
 * super-step ordinal; cetkmc_counters.supersteps counts these super-steps too. */
typedef struct cetkmc_local_args {
    int64_t step0, n_steps;
    int32_t box;              /* 8 */
    double  defect_fraction;
    uint64_t seed;
    int32_t thermal_mode;     /* 0 or 1 */
    double  thermal_dt;
    int32_t max_events;       /* 1..64 */
    double  horizon_events;   /* > 0, may be +inf */
} cetkmc_local_args;
int cetkmc_run_supersteps_local(void* handle, const cetkmc_local_args* a, cetkmc_run_result* res, double* totals,
                                cetkmc_event* events /* [n][D][max_events] or NULL */, int64_t* n_executed,
                                double* dt_event, double* horizon, int64_t* n_capped);

int cetkmc_get_counters(void* handle, cetkmc_counters* out, int reset);

/* Grain clustering on the device (utils.get_clusters / dfs_cluster, utils.py:28-84): connected
 * components of occupied 14-stencil neighbours with misorientation < threshold, numbered 1.. in the
 * order of their first voxel (row-major), exactly like the reference.  Whole lattice in one slab only.
 * _stats: per cluster first voxel (i,j,k), voxel count, bounding box (imin,jmin,kmin,imax,jmax,kmax);
 * _labels: the (L,L,L) int32 label volume the reference returns as `visited`. */
int cetkmc_cluster(void* handle, double threshold, int64_t* n_clusters);
int cetkmc_cluster_stats(void* handle, int64_t cap, int32_t* first_voxel, int64_t* size, int32_t* bbox);
int cetkmc_cluster_labels(void* handle, int32_t* labels);

/* Sparse site queries so that the host-side defect model (defects.track_defects, defects.py:4-19) and the
 * species counts of the metrics row (kmc_simulation.py:355-357) need no full-lattice transfer:
 * counts[s] = owned voxels in state s (0..4; [5] = other); gather: global linear index ((i*L+j)*L+k) and T of
 * every owned voxel of the given species (unordered, *n = total found; at most cap are written);
 * set_defects_sparse: defects := 0, then 1 at the listed voxels. */
int cetkmc_species_counts(void* handle, int64_t counts[6]);
int cetkmc_gather_species(void* handle, int species, int64_t* lin_idx, double* T_vals, int64_t cap, int64_t* n);
int cetkmc_set_defects_sparse(void* handle, const int64_t* lin_idx, int64_t n);

/* The nucleation count is the handle's running total over every stepping call and cetkmc_apply since creation.  It belongs
 * to the handle, not to the lattice: cetkmc_upload -- a whole new lattice included -- leaves it and cetkmc_counters as they
 * are.  cetkmc_reset_counters zeroes the step state, the nucleation count with it, and leaves cetkmc_counters alone;
 * cetkmc_get_counters(reset = 1) zeroes cetkmc_counters and leaves the nucleation count alone.  Neither touches the
 * lattice or any cached rate (tests/test_gpu_live_handle_vs_oracle.py pins all of this). */
int64_t cetkmc_nucleation_count(void* handle);
int cetkmc_reset_counters(void* handle);

/* Measurement helpers (bench.py): n back-to-back rate sweeps timed with hipEvents on the
 * engine's stream; returns total milliseconds. */
int cetkmc_time_sweeps(void* handle, int n, double* ms_total);
/* bench helper: average elapsed time between two hipEvents recorded back to back on the handle's stream, with one empty
 * kernel between them (n pairs) -- what a hipEvent-bracketed kernel duration includes besides the kernel's own work */
int cetkmc_event_overhead(void* handle, int n, double* ms_avg);
/* Transport self-test of a multi-rank handle (collective: every rank calls it with the same `bytes`): patterned buffers
 * through the all-gather and the neighbour exchange the stepping loops use, verified on the host; a single-rank RCCL
 * communicator sends to itself.  times_us (may be NULL) receives the average wall time in microseconds of 20 further
 * all-gathers [0] and neighbour exchanges [1] of that size, stream synchronisation included.  Single-process handle: no-op. */
int cetkmc_comm_selftest(void* handle, int64_t bytes, double* times_us);

/* Replica ensembles: R independent lattices of the same edge L (1 <= L <= 128) on one GPU, each
 * with its own parameters, fields, defect mask, random streams and step state, advanced one Mode A step per launch
 * sequence.  Every replica follows exactly the trajectory a single handle would (full sweep every step; thermal_mode 0,
 * 1 or 2, the update every 20 global steps shared by all replicas).  A replica whose step ends in the termination branch
 * (status 1) freezes: later calls leave it as it is (fields, prev_state) and report it with status 1 and no steps.
 * res[r].full_sweeps = the replica's executed steps.
 *
 * thermal_mode 2 (laser source on plane L-1, latent heat with use_latent, as in cetkmc_run_args): the source planes come
 * in n_sets plane sets of n_q planes each, q_planes[n_sets][n_q][L*L] in host memory, copied to the device once per call.
 * Replica r reads set q_set[r] (q_set NULL: set r, and n_sets must equal R); replicas that share a scan share a set.  The
 * u-th temperature update of the call (the u-th global step g of the call with g % 20 == 0) reads plane u of every set.
 * A call is refused before anything is launched when n_q is smaller than its number of updates, when q_planes is NULL
 * with an update due, when q_set is NULL and n_sets != R, or when a q_set entry lies outside [0, n_sets).  res[r].q_used:
 * as on a single handle, the planes consumed by the replica's executed steps including the step it stopped in; 0 for a
 * replica that was frozen when the call began.
 *
 * cetkmc_create_ensemble: p[R] (one parameter set per replica).  The returned handle addresses replica 0 in the
 * per-lattice calls; cetkmc_destroy on it releases the whole ensemble.
 * cetkmc_ensemble_replica: the handle of replica r, accepted by every per-lattice call (upload, download, set_defects,
 * set_prev_state, thermal_cet, thermal_laser, rate_sweep, species_counts, gather_species, set_defects_sparse, nucleation_count, cluster*,
 * front_stats, layer_profile, grain_table, solid_read, solid_profile, origin_read, origin_census, origin_seq, origin_profile,
 * origin_absorb_events) except the
 * stepping calls (run_steps, run_supersteps, stage_inputs refuse it); it belongs to the ensemble (cetkmc_destroy refuses
 * it).  A single-lattice handle is refused.  Uploading a new lattice (state) into a frozen replica unfreezes it.
 * R is bounded by the grid (R * ceil(L / 4) <= 65535) and by the free device memory at creation.
 * cetkmc_run_ensemble: n_steps steps of every live replica from global step step0.  res[R]; totals[R][n_steps + 1]
 * (totals[r][s] = total rate of replica r's step s, [steps_done] = the terminating total); dt[R][n_steps] (may be NULL;
 * rng_mode 2 only): the time increment of each step from the counter uniform of key KEY_DT, as cetkmc_run_supersteps'
 * dt_event for box == L.  All per-replica arrays are row-major with replica-major rows. */
typedef struct cetkmc_ens_args {
    int64_t step0;
    int64_t n_steps;
    const double* defect_fraction;  /* [R] */
    const double* u_pick;           /* [R][n_steps]   rng_mode 0 */
    const double* u_defect;         /* [R][n_steps]   rng_mode 0; may be NULL when every defect_fraction is 0 */
    const double* u_np;             /* [R][np_stride] rng_mode 0 */
    int64_t np_stride;              /* rng_mode 0: >= n_steps * (L*L + 2), the worst case -- no replica can run short */
    const uint64_t* seed;           /* [R]            rng_mode 2 */
    int32_t rng_mode;               /* 0 (reference streams) or 2 (all counter based) */
    int32_t thermal_mode;           /* 0, 1 or 2 */
    double thermal_dt;
    const double* q_planes;         /* [n_sets][n_q][L*L] thermal_mode 2, host memory */
    int64_t n_q;                    /* planes per set */
    int32_t n_sets;
    const int32_t* q_set;           /* [R] plane set of each replica; NULL: set r for replica r (n_sets == R) */
    int32_t use_latent;             /* thermal_mode 2 */
} cetkmc_ens_args;

int cetkmc_create_ensemble(const cetkmc_params* p, int L, int R, int device_id, void** handle);
int cetkmc_ensemble_replica(void* handle, int r, void** replica);
int cetkmc_run_ensemble(void* handle, const cetkmc_ens_args* a, cetkmc_run_result* res, double* totals, double* dt);

/* Batched analysis of every replica (the metrics rows of run_kmc_ensemble) in a number of launches that does not depend
 * on R.  cetkmc_ensemble_analyze: grain clustering (as cetkmc_cluster, misorientation threshold), species counts (as
 * cetkmc_species_counts), the nucleation counts and, for species >= 0, the (index, T) gather of cetkmc_gather_species.
 * cetkmc_ensemble_analysis_data then copies the results of the last analysis, concatenated over replicas in replica
 * order: sum(n_clusters) entries of first voxel (i,j,k) / size / bounding box (clusters numbered as cetkmc_cluster_stats
 * does), labels [R][L^3], sum(n_gathered) gathered entries (unordered within a replica).  Any output may be NULL.
 * cetkmc_ensemble_set_defects_sparse: cetkmc_set_defects_sparse for every replica r with counts[r] >= 0, its indices the
 * next counts[r] entries of lin_idx (replicas with counts[r] < 0 are left alone). */
typedef struct cetkmc_ens_analysis {
    double threshold;               /* in: clustering misorientation threshold (radians) */
    int32_t species;                /* in: state gathered; -1: no gather */
    int32_t pad;
    int64_t* n_clusters;            /* [R] out */
    int64_t* species_counts;        /* [R][6] out */
    int64_t* nucleation_count;      /* [R] out */
    int64_t* n_gathered;            /* [R] out (species >= 0) */
} cetkmc_ens_analysis;

int cetkmc_ensemble_analyze(void* handle, cetkmc_ens_analysis* a);
int cetkmc_ensemble_analysis_data(void* handle, int32_t* first_voxel, int64_t* size, int32_t* bbox, int32_t* labels,
                                  int64_t* lin_idx, double* T_vals);
int cetkmc_ensemble_set_defects_sparse(void* handle, const int64_t* counts, const int64_t* lin_idx);

/* Solidification-front diagnostics (NOT in the reference): one streaming pass over T and state on the
 * device, nothing written to the lattice.  With inv_dx = 1 / voxel edge (computed by the host, like inv_dx2):
 *   front voxel: state != 0 and at least one of its six face neighbours INSIDE the lattice has state == 0;
 *   gradient component along an axis at index x: (T[x+1] - T[x-1]) * (0.5 * inv_dx) inside, (T[1] - T[0]) * inv_dx at
 *     x == 0, (T[L-1] - T[L-2]) * inv_dx at x == L-1, 0.0 when L == 1; G = sqrt(gi*gi + gj*gj + gk*gk), left to right;
 *   a front voxel whose G or own T is not finite is counted in n_skipped and in nothing else;
 *   melt voxel: any voxel, whatever its state, with T >= T_melt of the lattice's parameters (NaN is none, +inf is one).
 * The three sums are formed in a fixed order (no floating-point atomics): two calls on an unchanged lattice return the same
 * bits, and a replica's entry of the batched call has the bits of the same lattice on a single handle.
 * (A struct tag without a typedef: the per-lattice call carries the same name.) */
struct cetkmc_front_stats {
    int64_t n_front;        /* front voxels not skipped                                             */
    int64_t n_skipped;      /* front voxels skipped                                                 */
    int64_t pos_sum[3];     /* sum of i, j, k over the n_front voxels                               */
    double  G_sum, G_min, G_max;   /* over the n_front voxels; G_min = G_max = 0 when n_front == 0  */
    double  Gi_sum;         /* signed sum of gi, the component along the build direction (axis 0)   */
    double  T_sum;          /* sum of the front voxels' own T                                       */
    int64_t n_melt;         /* melt voxels                                                          */
    int32_t melt_bbox[6];   /* imin, jmin, kmin, imax, jmax, kmax of the melt voxels; {L, L, L, -1, -1, -1} when none */
};
/* One lattice: a single-slab, single-process handle or a replica handle (multi-slab and multi-rank handles are refused).
 * Ordered on the handle's stream behind pending stepping work; copies sizeof(struct cetkmc_front_stats) to the host. */
int cetkmc_front_stats(void* handle, double inv_dx, struct cetkmc_front_stats* out);
/* Every replica of an ensemble, frozen ones included, in a launch sequence that does not depend on R; out[R].  A
 * single-lattice handle is refused. */
int cetkmc_ensemble_front_stats(void* handle, double inv_dx, struct cetkmc_front_stats* out);

/* Layer-resolved grain structure (not in the reference): one record of integer counters per plane i
 * of the build direction (axis 0), from the label volume and the per-grain table of the handle's LAST clustering and the
 * lattice's state, in one streaming pass on the device.  g(v) is the label of voxel v = (i, j, k) (0 = empty, ids 1..n as
 * cetkmc_cluster_stats / _labels number them), s(v) its state.  Only voxels with g(v) != 0 count, each in the record of its
 * own plane:
 *   n_occ        +1;
 *   n_start      +1 if v is its grain's first voxel in row-major order;
 *   n_eq         +1 if its grain is equiaxed: (double)max(d) / (double)max(min(d), 1) < ar_threshold over the extents
 *                d = max - min + 1 of the grain's bounding box (the expression of metrics.compute_metrics_from_clusters);
 *   seg[a]       +1 if the predecessor u of v along axis a (that coordinate minus 1) is outside the lattice or
 *                g(u) != g(v): a grain segment of a line along axis a starts here;
 *   cut[a]       +1 if u is inside, g(u) != 0 and g(u) != g(v): a grain-grain boundary crossed by that line;
 *   occ_state[t-1]  +1 for t = s(v) in 1..4;
 *   gb_state[t-1]   +1 if in addition one of the six face neighbours of v inside the lattice has a label other than g(v)
 *                (label 0 counts as other): metrics.compute_boundary_fraction's rule with grain_ids = labels.
 * Everything is integer counting: the result is defined to the bit.  pad is 0.
 * The profile describes the lattice as it was clustered: for a lattice changed since that clustering (stepping, uploads)
 * the result is unspecified (the call stays inside its arrays).
 * (A struct tag without a typedef, as cetkmc_front_stats.) */
struct cetkmc_layer_rec {
    int64_t n_occ, n_start, n_eq;
    int64_t seg[3], cut[3];
    int64_t occ_state[4], gb_state[4];
    int64_t pad;
};
/* One lattice: a single-slab, single-process handle or a replica handle, after cetkmc_cluster on that handle (without
 * one the call fails as cetkmc_cluster_labels does; multi-slab and multi-rank handles are refused).  The handle
 * cetkmc_create_ensemble returned is refused here although it addresses replica 0 elsewhere: replica 0's profile is entry 0
 * of the batched call.  out[L].  Ordered on the handle's stream behind pending stepping work; copies
 * L * sizeof(struct cetkmc_layer_rec) to the host (counted in bytes_d2h); writes no lattice field. */
int cetkmc_layer_profile(void* handle, double ar_threshold, struct cetkmc_layer_rec* out);
/* Every replica of an ensemble, frozen ones included, from the clustering of the last cetkmc_ensemble_analyze (required),
 * in a launch sequence that does not depend on R; out[R][L].  A single-lattice handle is refused. */
int cetkmc_ensemble_layer_profile(void* handle, double ar_threshold, struct cetkmc_layer_rec* out);

/* Imported labellings: install a labelling of the caller's as the handle's last clustering, exactly
 * as cetkmc_cluster would have left it (labels, first voxels ascending, size / bounding-box table, cluster count), so that
 * cetkmc_cluster_stats, cetkmc_cluster_labels and cetkmc_layer_profile read it; a later cetkmc_cluster replaces it
 * completely.  labels[L^3], row-major: 0 = empty, ids 1..n numbered by first occurrence in row-major order (so every id
 * 1..n is present); a grain need not be connected.  Anything else is refused on the host with a message that names the
 * offending voxel, before anything is allocated, uploaded or launched: the profile kernel indexes its tables with the
 * label.  Labels are not checked against the lattice's state: the counters follow their definition, occupancy from the
 * labels and species from the state.  A single-slab, single-process handle or a replica handle; multi-slab and multi-rank
 * handles and the handle cetkmc_create_ensemble returned are refused. */
int cetkmc_cluster_import(void* handle, const int32_t* labels, int64_t* n_clusters);
/* The same for every replica of an ensemble, in place of the clustering of the last cetkmc_ensemble_analyze (required: its
 * species counts and gather results stay as they are): labels[R][L^3], n_clusters[R] out.  Every replica is checked before
 * anything is uploaded; one bad replica refuses the call and leaves the previous analysis intact.
 * cetkmc_ensemble_analysis_data and cetkmc_ensemble_layer_profile then read the import.  A single-lattice handle is refused. */
int cetkmc_ensemble_cluster_import(void* handle, const int32_t* labels, int64_t* n_clusters);

/* Grain-boundary misorientation and texture profiles (not in the reference): integer histograms per
 * plane i of the build direction (axis 0), from the label volume of the handle's LAST clustering (cetkmc_cluster or
 * cetkmc_cluster_import) and the per-voxel orientation unit vectors the device keeps (sin t cos p, sin t sin p, cos t), in
 * one streaming pass.  g(v) is the label of voxel v = (i, j, k) (0 = empty), o(v) its three doubles.
 * One binning rule serves both histograms: over n_bins - 1 interior edges e[0] > e[1] > ... (strictly decreasing, finite:
 * cosines of ascending angles, computed by the caller) bin(x) is the number of edges with x <= e[q], so bin 0 holds the
 * values above e[0] and bin n_bins - 1 those at or below the last edge.  The device applies no acos and no clamp (a value
 * above 1 by rounding lands in bin 0); a value that is not finite is counted in bad and in no bin.
 *   gb_hist[i][a][b]   for every v of plane i with g(v) != 0 and every axis a whose predecessor u (that coordinate minus 1)
 *                      is inside the lattice with g(u) != 0 and g(u) != g(v) -- the faces cut[a] of cetkmc_layer_rec counts:
 *                      +1 at b = bin(d), d = o(u)[0]*o(v)[0] + o(u)[1]*o(v)[1] + o(u)[2]*o(v)[2] summed left to right
 *                      without fused multiply-add, against gb_edges; bad[i][a] +1 instead if d is not finite;
 *   pole_hist[i][b]    for every v of plane i with g(v) != 0: +1 at b = bin(c), c = fabs(axis[0]*o(v)[0] + axis[1]*o(v)[1]
 *                      + axis[2]*o(v)[2]) against pole_edges; bad[i][3] +1 instead if c is not finite.
 * axis is used as given (not normalised) and must be finite.  So sum_b gb_hist[i][a][b] + bad[i][a] == cut[a] and
 * sum_b pole_hist[i][b] + bad[i][3] == n_occ of plane i's cetkmc_layer_rec.  Everything is integer counting: the result is
 * defined to the bit given the vectors, and two calls return the same bits.  For a lattice changed since its clustering the
 * result is unspecified (the call stays inside its arrays). */
struct cetkmc_texture_args {
    int32_t n_bins;               /* 1..64, of both histograms                                             */
    int32_t pad;
    const double* gb_edges;       /* [n_bins - 1] host, strictly decreasing; may be NULL when n_bins == 1  */
    const double* pole_edges;     /* [n_bins - 1] likewise                                                 */
    double axis[3];
};
/* One lattice, under the handle rules of cetkmc_layer_profile.  gb_hist[L][3][n_bins], pole_hist[L][n_bins], bad[L][4]; any
 * of the three may be NULL.  n_bins outside 1..64, a NULL edge array with n_bins > 1, an edge that is not finite or not
 * below its predecessor and a non-finite axis are refused on the host before anything is allocated or launched.  Ordered on
 * the handle's stream behind pending stepping work; copies L * (4 * n_bins + 4) * 8 bytes to the host (counted in
 * bytes_d2h); writes no lattice field. */
int cetkmc_texture_profile(void* handle, const struct cetkmc_texture_args* args, int64_t* gb_hist, int64_t* pole_hist, int64_t* bad);
/* Every replica of an ensemble, frozen ones included, from the clustering of the last cetkmc_ensemble_analyze (required) or
 * an import on top of it, in one launch whatever R; gb_hist[R][L][3][n_bins], pole_hist[R][L][n_bins], bad[R][L][4].  A
 * single-lattice handle is refused. */
int cetkmc_ensemble_texture_profile(void* handle, const struct cetkmc_texture_args* args, int64_t* gb_hist, int64_t* pole_hist,
                                    int64_t* bad);

/* Per-grain table (not in the reference): one record per grain id 1..n of the handle's LAST clustering
 * (cetkmc_cluster or cetkmc_cluster_import), from the label volume g, the lattice's state s and the stored angles, in one
 * streaming pass on the device.  Entry id - 1 is fed by every voxel v = (i, j, k) with g(v) == id:
 *   n            +1 (equals the size cetkmc_cluster_stats reports);
 *   sum[a]       + the coordinate a of v (i, j, k);
 *   sq[..]       + i*i, j*j, k*k, i*j, i*k, j*k;
 *   n_state[t-1] +1 for t = s(v) in 1..4 (a labelled voxel with another state is in none);
 *   nb_*         for each of the 14 stencil offsets d of the clustering (kmc_event_rates.py:29-35), u = v + d:
 *                u outside the lattice -> nb_out; g(u) == 0 -> nb_empty; g(u) == g(v) -> nb_same; otherwise -> nb_other.
 * So nb_same + nb_other + nb_empty + nb_out == 14 * n, and the sum of nb_same over the grains is even.  first_theta and
 * first_phi are the stored angles of the grain's first voxel in row-major order, copied bit for bit.  The 18 counters are
 * integer sums (no floating point in the voxel pass, no floating-point atomics): the record is defined to the bit and two
 * calls return the same bits.  For a lattice changed since its clustering the result is unspecified (the call stays inside
 * its arrays).  (A struct tag without a typedef, as cetkmc_layer_rec.) */
struct cetkmc_grain_rec {
    int64_t n;
    int64_t sum[3];
    int64_t sq[6];
    int64_t n_state[4];
    int64_t nb_same, nb_other, nb_empty, nb_out;
    double  first_theta, first_phi;
};
/* One lattice, under the handle rules of cetkmc_layer_profile (the handle cetkmc_create_ensemble returned, multi-slab and
 * multi-rank handles are refused; without a clustering the call fails as cetkmc_cluster_labels does).  out[min(cap, n)]: the
 * first min(cap, n) records, as cetkmc_cluster_stats treats cap.  Every refusal happens before anything is allocated or
 * launched; a device allocation that fails is reported through cetkmc_last_error and leaves the handle usable.  Ordered on
 * the handle's stream behind pending stepping work; copies min(cap, n) * sizeof(struct cetkmc_grain_rec) to the host
 * (counted in bytes_d2h); writes no lattice field. */
int cetkmc_grain_table(void* handle, int64_t cap, struct cetkmc_grain_rec* out);
/* Every replica of an ensemble, frozen ones included, from the clustering of the last cetkmc_ensemble_analyze (required) or
 * an import on top of it, in a launch sequence that does not depend on R: out[sum of n_clusters], the replicas' records one
 * behind the other in replica order.  A single-lattice handle is refused. */
int cetkmc_ensemble_grain_table(void* handle, struct cetkmc_grain_rec* out);

/* Solidification map (not in the reference): the thermal conditions at a voxel WHEN IT SOLIDIFIED,
 * kept on the device between stepping calls, and a profile call that reduces them per build plane and per grain.
 * The map of a handle holds, per voxel of the (L, L, L) lattice (row-major, axis 0 = build direction), stamp (int64, -1 = no
 * record) and five doubles T_s, gi, gj, gk, cool, plus a private snapshot of the state bytes and of T.
 *   cetkmc_solid_begin   allocates the map, sets stamp = -1 and the doubles to +0.0 everywhere and snapshots the current state
 *                        and T.  Voxels occupied now are substrate: they have no record.  A second begin resets the map.
 *   cetkmc_solid_end     frees it.  Every other solid call without a map is refused.
 *   cetkmc_solid_update  stamp >= 0, dt finite and > 0, inv_dx finite (anything else is refused on the host before a launch).
 *     For every voxel v with snapshot state s0 and current state s1:
 *       s0 == 0 && s1 != 0 (solidified since the last update): stamp(v) = stamp; T_s = T(v); gi, gj, gk = the gradient
 *         components of cetkmc_front_stats exactly ((T[x+1] - T[x-1]) * (0.5 * inv_dx) inside, (T[1] - T[0]) * inv_dx at
 *         x == 0, (T[L-1] - T[L-2]) * inv_dx at x == L-1, 0.0 when L == 1); cool = (T(v) - T_snap(v)) / dt -- no contraction,
 *         IEEE division, non-finite results stored as they come; info.n_new += 1;
 *       s0 != 0 && s1 == 0 (remelted, or hopped away): stamp = -1, the five doubles = +0.0; info.n_cleared += 1 (a substrate
 *         voxel that empties counts here too);
 *       anything else, a change of species included: the record is untouched.
 *     Then snapshot = state and T_snap = T for every voxel.  info.n_recorded = voxels with stamp >= 0 after the call.  A voxel
 *     that solidifies and empties again between two updates is not seen.  The call reads the lattice as it stands (the
 *     current buffer of the T pair, behind pending stepping work on the handle's stream), writes no lattice field and touches
 *     no cached rate, list, row sum or staged batch.  info may be NULL.
 *   cetkmc_solid_read    copies the map: stamp[L^3], T_s[L^3], g[L^3][3], cool[L^3]; any pointer may be NULL; counted in
 *                        bytes_d2h.
 *   cetkmc_solid_profile one record per plane i (layers[L]) and per grain id of the handle's last clustering (grains, the
 *     first min(cap, n) records as cetkmc_grain_table treats cap; grains == NULL: no clustering is needed).  The four
 *     quantities x0 = G = sqrt(gi*gi + gj*gj + gk*gk) (left to right), x1 = gi, x2 = cool, x3 = T_s are quantised with
 *     qscale[c] (finite and > 0, otherwise refused).  A voxel with stamp >= 0 is GOOD when all four x are finite and every
 *     |x_c * qscale[c]| < 2^38 (with L^3 <= 2^24 the sums stay inside int64).  A good voxel adds n_rec +1, stamp_sum + stamp,
 *     stamp_min / stamp_max, q[c] += llrint(x_c * qscale[c]) (round to nearest even), n_cooling +1 if cool < 0; any other
 *     recorded voxel adds n_bad +1 and nothing else.  A record without a good voxel has stamp_min = INT64_MAX and
 *     stamp_max = -1.  A recorded voxel with label 0 counts in its plane only.  Everything in the reduction is integer
 *     arithmetic (integer atomics): the result is defined to the bit given the map.  For a lattice changed since its
 *     clustering the result is unspecified (the call stays inside its arrays).
 * Handles: a single-slab, single-process handle.  begin / update / end refuse a handle that belongs to an ensemble (the
 * batched calls keep every replica's map); read and profile take a replica handle; profile refuses the handle
 * cetkmc_create_ensemble returned, as cetkmc_layer_profile does.  Multi-slab and multi-rank handles are refused.  Every
 * refusal happens before anything is allocated or launched; a device allocation that fails is reported through
 * cetkmc_last_error and leaves the handle usable (without a map).  cetkmc_destroy frees the map.
 * (Struct tags without typedefs, as cetkmc_grain_rec.) */
struct cetkmc_solid_info { int64_t n_new, n_cleared, n_recorded; };
struct cetkmc_solid_args { double qscale[4]; };
struct cetkmc_solid_rec {
    int64_t n_rec, n_bad, n_cooling;
    int64_t stamp_sum, stamp_min, stamp_max;
    int64_t q[4];             /* quantised sums of G, gi, cool, T_s over the n_rec good voxels */
};
int cetkmc_solid_begin(void* handle);
int cetkmc_solid_end(void* handle);
int cetkmc_solid_update(void* handle, int64_t stamp, double inv_dx, double dt, struct cetkmc_solid_info* info);
int cetkmc_solid_read(void* handle, int64_t* stamp, double* T_s, double* g, double* cool);
int cetkmc_solid_profile(void* handle, const struct cetkmc_solid_args* args, struct cetkmc_solid_rec* layers, int64_t cap,
                         struct cetkmc_solid_rec* grains);
/* Every replica of an ensemble, frozen ones included (nothing changes in them; their snapshots are refreshed), in a launch
 * sequence that does not depend on R.  stamp, inv_dx and dt are shared; info[R]; layers[R][L]; grains: the replicas' records
 * one behind the other in replica order, as cetkmc_ensemble_grain_table lays them out (NULL: no clustering is needed;
 * otherwise the clustering of the last cetkmc_ensemble_analyze or an import on top of it is required).  A replica's bits
 * equal those of the same lattice on a single handle.  A single-lattice handle is refused. */
int cetkmc_ensemble_solid_begin(void* handle);
int cetkmc_ensemble_solid_end(void* handle);
int cetkmc_ensemble_solid_update(void* handle, int64_t stamp, double inv_dx, double dt, struct cetkmc_solid_info* info);
int cetkmc_ensemble_solid_profile(void* handle, const struct cetkmc_solid_args* args, struct cetkmc_solid_rec* layers,
                                  struct cetkmc_solid_rec* grains);

/* Origin map (not in the reference): HOW and WHEN each voxel was last filled -- by deposition,
 * nucleation, attachment to an existing grain or a diffusion hop -- kept on the device and fed from the event log every
 * stepping call already writes there, and a profile call that reduces it per build plane and per grain.
 * Map: per voxel of the (L, L, L) lattice (row-major, axis 0 = build direction) one uint64 word.  0 = no record; otherwise
 *   ((ordinal + 1) << 3) | code with code 1 DEP, 2 NUC, 3 ATT, 4 HOP (a diffusion arrived here), 5 LEFT (a diffusion left
 *   here).  Codes 1..4 are the fill codes.
 * Ordinal: the map has its own clock seq, 0 at cetkmc_origin_begin, never going back.  A Mode A call (cetkmc_run_steps,
 *   cetkmc_run_ensemble per replica, cetkmc_run_supersteps with box == L) that executed steps_done steps gives slot s of its
 *   log the ordinal seq + s and advances seq by steps_done; a Mode B call gives every record of super-step t the ordinal
 *   seq + t (the events of one super-step never touch the same voxel) and advances seq by its executed super-steps;
 *   cetkmc_apply uses one ordinal.  The map does not depend on the caller's step0.  A call that could take seq to 2^36 or
 *   beyond is refused before it does anything.
 * Absorbing one record (cetkmc_event) with ordinal o, enc(o, code) = ((o + 1) << 3) | code:
 *   type outside 0..3 (idle -1, null -2): skipped;
 *   dep, nuc, att: word(pos) = max(word(pos), enc(o, DEP / NUC / ATT));
 *   diff with target[0] >= 0: word(pos) = max(word(pos), enc(o, LEFT)), word(target) = max(word(target), enc(o, HOP));
 *   a diff with target[0] < 0 is skipped.
 *   "Later wins" is this maximum, so the result does not depend on the order in which records are processed.  A hop does
 *   not carry the moved atom's provenance: it becomes HOP (the profile counts these).  Defect injection changes no code.
 * Census: int64 census[L][5], running since begin: every absorbed record adds 1 at [pos[0]][type] (0 dep, 1 diff, 2 nuc,
 *   3 att), a diffusion also at [target[0]][4].  It counts events whether or not a later one overwrote the voxel: column 2
 *   is the nucleation-rate profile along the build axis.
 * While a map exists cetkmc_run_steps absorbs slots [0, steps_done) of its log, cetkmc_run_supersteps its done x D records
 * (single-process handles), cetkmc_run_supersteps_local its done x D x max_events records (several records of one voxel
 * under one ordinal resolve by the maximum like any others: by the code, not by their sequence), cetkmc_run_ensemble every replica's executed steps and cetkmc_apply its event; the slot of a
 * step that terminated (status 1) or ran out of its stream (status 2) is not absorbed.  The absorbing launch follows the
 * call's closing event on the handle's stream: wall_ms and the counters do not include it, and no stepping kernel changes.
 * Uploads, defect masks and temperature updates are no events: an upload is simply not recorded (its atoms are unrecorded).
 * The origin calls invalidate no cache of the handle, and nothing invalidates the map.
 *   cetkmc_origin_begin   allocates the map (words and census 0, seq 0); a second begin resets it.  L > 256 is refused.
 *   cetkmc_origin_end     frees it.  Every other origin call without a map is refused (cetkmc_origin_seq returns -1).
 *   cetkmc_origin_absorb_events  n host records, records [g * group, (g + 1) * group) with ordinal seq + g; seq advances by
 *                         n / group.  group >= 1, n >= 0 and n % group == 0; an event (type 0..3) whose position, or a
 *                         diffusion whose target with target[0] >= 0, lies outside the lattice refuses the call.
 *   cetkmc_origin_read    words[L^3];  cetkmc_origin_census  out[L][5];  both counted in bytes_d2h.
 *   cetkmc_origin_profile one record per plane i (layers[L]) and per grain id of the handle's last clustering
 *     (cetkmc_cluster or cetkmc_cluster_import; grains: the first min(cap, n) records as cetkmc_grain_table treats cap;
 *     grains == NULL: no clustering is needed).
 *     Plane record: a voxel with state != 0 counts in n_occ and in n_by[code - 1] if its word has a fill code, otherwise
 *       (word 0 or LEFT) in n_unrec; a voxel with state == 0 and code LEFT counts in n_left; any other empty voxel in nothing.
 *     Grain record: every voxel with label == id counts in n_occ and is classified by its word alone, as above (labels are
 *       not checked against the state); n_left is 0.
 *     Over the voxels counted with a fill code: ord_sum, ord_min, ord_max over their ordinals; birth = the minimum of
 *       (ordinal << 27) | (code << 24) | lin with lin = (i * L + j) * L + k -- the earliest fill, ties (Mode B) broken by code
 *       and then by position.  A record without such a voxel has ord_min = birth = INT64_MAX and ord_max = -1.  pad is 0.
 *     Integer add / min / max only: the result is defined to the bit, two calls return the same bytes and a replica's bytes
 *     equal those of the same lattice on a single handle.  For a lattice changed since its clustering the result is
 *     unspecified (the call stays inside its arrays).
 * Handles: a single-slab, single-process handle.  begin / end refuse a handle that belongs to an ensemble (the batched calls
 * keep every replica's map); read, census, seq, profile and absorb_events take a replica handle; profile refuses the handle
 * cetkmc_create_ensemble returned, as cetkmc_layer_profile does.  Multi-slab and multi-rank handles are refused.  Every
 * refusal happens before anything is allocated or launched; a device allocation that fails is reported through
 * cetkmc_last_error and leaves the handle usable.  cetkmc_destroy frees the map.
 * (A struct tag without a typedef, as cetkmc_grain_rec.) */
enum { CETKMC_ORIGIN_DEP = 1, CETKMC_ORIGIN_NUC = 2, CETKMC_ORIGIN_ATT = 3, CETKMC_ORIGIN_HOP = 4, CETKMC_ORIGIN_LEFT = 5 };
struct cetkmc_origin_rec {
    int64_t n_occ;
    int64_t n_by[4];          /* DEP, NUC, ATT, HOP */
    int64_t n_unrec, n_left;
    int64_t ord_sum, ord_min, ord_max;
    int64_t birth;
    int64_t pad;
};
int cetkmc_origin_begin(void* handle);
int cetkmc_origin_end(void* handle);
int cetkmc_origin_absorb_events(void* handle, const cetkmc_event* ev, int64_t n, int64_t group);
int cetkmc_origin_read(void* handle, uint64_t* words);
int cetkmc_origin_census(void* handle, int64_t* out);
int64_t cetkmc_origin_seq(void* handle);
int cetkmc_origin_profile(void* handle, struct cetkmc_origin_rec* layers, int64_t cap, struct cetkmc_origin_rec* grains);
/* Every replica of an ensemble, frozen ones included, in a launch sequence that does not depend on R.  census out[R][L][5];
 * layers[R][L]; grains: the replicas' records one behind the other in replica order, as cetkmc_ensemble_grain_table lays
 * them out (NULL: no clustering is needed; otherwise the clustering of the last cetkmc_ensemble_analyze or an import on top
 * of it is required).  A single-lattice handle is refused. */
int cetkmc_ensemble_origin_begin(void* handle);
int cetkmc_ensemble_origin_end(void* handle);
int cetkmc_ensemble_origin_census(void* handle, int64_t* out);
int cetkmc_ensemble_origin_profile(void* handle, struct cetkmc_origin_rec* layers, struct cetkmc_origin_rec* grains);

/* Remelting (not in the reference, which has no melting): solid at or above a threshold temperature
 * turns liquid.  Opt-in; while it is off every launch and byte of a stepping call is what it was without it.
 * One pass over the lattice, with m = (state != 0) & (T >= threshold) -- a NaN temperature never melts, +inf does, equality
 * melts, a state-4 voxel (a defect written into the state) melts like an atom:
 *   on m: state = 0, prev_state = 0, theta = phi = 0.0 (the voxel is written as the reference's own "site empties" write,
 *   kmc_simulation.py:286-290).  prev_state is cleared so that a voxel that melts and refills before the next laser update
 *   releases latent heat (thermal_solver.py:98).  Nothing else changes: the defect MASK, T, empty voxels and their
 *   orientations, the nucleation count and cetkmc_counters stay.  No heat is absorbed (the reference's latent term is
 *   release-only).  A pass is idempotent on an unchanged field.
 * The voxels of the rows around a melted voxel are relisted (interface list, neighbourhood words), not evaluated.
 *   cetkmc_remelt      one pass now, behind the pending work of the handle's stream; a single handle or a replica handle.
 *                      It costs what cetkmc_apply costs (cause "apply" of cetkmc_invalidates: the row sums and the interface
 *                      sums go stale, the rate table stays valid).  A pass that melts nothing -- threshold +inf, or nothing hot
 *                      enough -- leaves the lattice as it is, and is a pass all the same: it is counted and raises the same
 *                      cause.  info may be NULL.  On a replica that has terminated the pass
 *                      may create events, but the replica stays frozen for cetkmc_run_ensemble until a lattice is uploaded
 *                      into it, as after any other change of a terminated replica.
 *   cetkmc_time_remelt n passes bracketed by one hipEvent pair on the handle's stream (ms_total; as cetkmc_time_sweeps times
 *                      sweeps), then one untimed cetkmc_remelt: measurement only (tools/remelt_timing.py).  The lattice is
 *                      what ONE pass leaves (the rule is idempotent); cetkmc_remelt_info.passes grows by n + 1 and
 *                      n_melted_last is the untimed pass's count, 0 when n >= 1.
 *   cetkmc_set_remelt  on != 0: every temperature-update step (g % 20 == 0, thermal_mode 1 or 2) of cetkmc_run_steps runs a
 *                      pass behind the update (and behind its prev_state := state) and before that step's rate evaluation.
 *                      Nothing happens with thermal_mode 0.  Behind an early stop (status 1 or 2) the queued passes are
 *                      pass-throughs, as the temperature kernels are; the continuation of a batch that stopped with status 2
 *                      ON an update step skips the pass together with the update it skips, so it is counted once.  The call
 *                      invalidates no cache and involves no cetkmc_set_option key.
 *   cetkmc_get_remelt_info   the handle's counters as last read from the device: at the end of a stepping call made while
 *                      remelting is on (with its results, no extra synchronisation inside a batch; a call made while it is
 *                      off copies nothing, also on a handle that used remelting before) and at the end of cetkmc_remelt.
 *   cetkmc_ensemble_set_remelt / cetkmc_ensemble_remelt_info   the same for cetkmc_run_ensemble, one threshold (T_melt is
 *                      shared by the replicas), info[R]; the launch sequence does not depend on R; a replica that has
 *                      terminated or is frozen is left alone.  A replica's bits equal those of a single handle.
 * cetkmc_remelt_info: running totals on the handle since its creation (direct passes and passes of the stepping loop alike)
 *   -- passes, n_melted, n_appended (voxels a pass added to the interface list) -- and n_melted_last, the last pass's count.
 * Refused, before anything is launched: a NaN threshold; a handle with more than one slab or a rank handle (the halo copies
 * would need the neighbour's field); cetkmc_set_remelt on an ensemble's handles (cetkmc_ensemble_set_remelt switches them)
 * and with option thermal_lookahead on; cetkmc_remelt and switching on while an origin map is attached (the event log it
 * folds holds no melts).  While remelting is on: cetkmc_run_supersteps, cetkmc_run_supersteps_local, option
 * thermal_lookahead = 1, cetkmc_origin_begin and cetkmc_ensemble_origin_begin are refused.  The solidification map needs
 * nothing: it sees occupied -> empty at its next update.
 * (A struct tag without a typedef, as cetkmc_grain_rec.) */
struct cetkmc_remelt_info { int64_t passes, n_melted, n_melted_last, n_appended; };
int cetkmc_set_remelt(void* handle, int on, double threshold);
int cetkmc_remelt(void* handle, double threshold, struct cetkmc_remelt_info* info);
int cetkmc_time_remelt(void* handle, double threshold, int n, double* ms_total);
int cetkmc_get_remelt_info(void* handle, struct cetkmc_remelt_info* info);
int cetkmc_ensemble_set_remelt(void* handle, int on, double threshold);
int cetkmc_ensemble_remelt_info(void* handle, struct cetkmc_remelt_info* info);

/* ---- sub-stepped temperature updates -------------------------------------------------------------
 * The explicit update is stable only for alpha dt / dx^2 <= 1/6; the reference's dt = 1e-6 s gives 2.716.  With
 * thermal_substeps = n >= 1 (default 1: nothing changes) EVERY temperature update the handle performs -- cetkmc_thermal_cet,
 * cetkmc_thermal_laser, the cadence updates of cetkmc_run_steps and cetkmc_run_ensemble -- is n consecutive applications of
 * the existing update with dt_s = dt / n (one IEEE division on the host), all from the same source plane, clipped after
 * each.  Sub-step 1 is the existing launch: NaN scrub, latent-heat term, prev_state := state, row flags cleared.  Sub-steps
 * 2..n have neither scrub nor latent term.  One update still consumes one source plane, counts once in
 * cetkmc_counters.thermal_updates, and is applied or skipped as a whole (the marker of a status-2 stop, the pass-through
 * behind a terminated batch); with remelting on, the melt pass follows the last sub-step.
 *   cetkmc_set_thermal_substeps            a single handle (not a rank handle, not an ensemble's handles)
 *   cetkmc_ensemble_set_thermal_substeps   an ensemble handle: one n for all replicas (they share the thermal settings)
 *   cetkmc_get_substep_info                running totals of the handle since its creation: updates made while n > 1,
 *                      their sub-steps, the temperature-kernel launches they took, and how many of those were the
 *                      temporally blocked k_thermal_sub (thermal_sub.hpp) -- which proves which kernel ran.  An ensemble
 *                      handle reports the launches of its calls (one launch steps all replicas).
 *   cetkmc_time_thermal                    n_updates updates with dt = 1e-6 s and the scrub (laser != 0: with the handle's last
 *                      cetkmc_thermal_laser plane, zeros before the first, and the latent-heat term) bracketed by one hipEvent pair on the
 *                      handle's stream: measurement only (tools/thermal_substeps_timing.py).  The updates are real: afterwards
 *                      the handle's field has advanced by n_updates updates (each of thermal_substeps sub-steps; in laser
 *                      mode prev_state := state as well), with what any direct update makes stale (cause "thermal_update").
 * On a handle with one slab sub-steps 2..n can run in k_thermal_sub, option "substep_block" sub-steps per launch: 2..4; 1 =
 * the plain path (n launches of the existing kernel); 0 = the measured default, 3 at L > 128 and the plain path up to
 * L = 128, where it is faster.  A handle with several in-process slabs and an ensemble take the plain path.  Option
 * "substep_planes" sets the planes per block of k_thermal_sub (0 = chosen so that the blocks fill the device once).  Same
 * bits either way.
 * Refused, before anything is launched: n < 1 and n > 65536 (the launch bookkeeping is int); rank handles
 * (cetkmc_create_rank*); n > 1 while option thermal_lookahead is on, and thermal_lookahead = 1 while n > 1;
 * cetkmc_set_thermal_substeps on an ensemble's own handle or on its replicas; cetkmc_run_supersteps and
 * cetkmc_run_supersteps_local while n > 1 (Mode B is out of scope). */
#define CETKMC_MAX_THERMAL_SUBSTEPS 65536
struct cetkmc_substep_info { int64_t updates, substeps, launches, blocked_launches; };
int cetkmc_set_thermal_substeps(void* handle, int n);
int cetkmc_ensemble_set_thermal_substeps(void* handle, int n);
int cetkmc_get_substep_info(void* handle, struct cetkmc_substep_info* info);
int cetkmc_time_thermal(void* handle, int laser, int n_updates, double* ms_total);

/* ---- implicit temperature updates ------------------------------------------------------------------
 * An opt-in, unconditionally stable scheme for EVERY temperature update the handle performs (the direct calls, the cadence
 * updates of cetkmc_run_steps and cetkmc_run_ensemble, cetkmc_time_thermal): a locally one-dimensional backward-Euler step.
 * With the scheme CETKMC_THERMAL_EXPLICIT (the default) nothing changes.  One implicit step of length dt:
 *   1. b = tc + dt * (qterm + latent_coef * dF) per voxel, thermal_voxel()'s terms without the Laplacian; tc = scrub(T), where
 *      the scrub of this scheme maps NaN -> T_nan, +inf -> T_clip_hi, -inf -> T_clip_lo and leaves finite values alone;
 *   2. (I - r D) x = b along every line of axis 2, then of axis 1, then of axis 0; r = (alpha * dt) * inv_dx2; D the 1-D second
 *      difference with the lattice edge replicated (diagonal 1 + r at both ends, 1 + 2 r inside, off-diagonals -r; L = 1: the
 *      identity).  Thomas algorithm with the coefficients of cetkmc_implicit_coeffs:
 *        inv[0] = 1 / (1 + r) (L = 1: 1), p[0] = r * inv[0];  beta = ((m < L - 1) ? (1 + 2 r) : (1 + r)) - r * p[m - 1],
 *        inv[m] = 1 / beta, p[m] = r * inv[m];
 *        y[0] = b[0] * inv[0], y[m] = (b[m] + r * y[m - 1]) * inv[m];  x[L - 1] = y[L - 1], x[m] = y[m] + p[m] * x[m + 1];
 *   3. the clip to [T_clip_lo, T_clip_hi], once, after the third solve;
 *   4. with the latent term on: prev_state := state, row flags cleared.
 * thermal_substeps = n composes: an update is n implicit steps of dt / n; step 1 carries the scrub and the latent term, all
 * use the same source plane; one update consumes one plane, counts once, and is applied or skipped as a whole.
 *   cetkmc_set_thermal_scheme            a single handle; leaves every cache and the applied-update marker alone
 *   cetkmc_ensemble_set_thermal_scheme   an ensemble handle: one scheme for all replicas
 *   cetkmc_get_implicit_info             running totals: implicit updates, their steps, their kernel launches (three per step:
 *                      k_imp_rows, k_imp_lines<1>, k_imp_lines<0>, thermal_imp.hpp), and rebuilds of the device's coefficient
 *                      table (one per change of r).  cetkmc_substep_info counts explicit updates only.
 *   cetkmc_implicit_coeffs               the host routine that fills the table; needs no device.  Refuses L < 1, a non-finite r
 *                      and r < 0.
 * Refused, before anything is allocated or launched: an unknown scheme; cetkmc_set_thermal_scheme on an ensemble's handle or on
 * its replicas; the implicit scheme on a handle with several slabs and on rank handles (the solve along axis 0 crosses slabs);
 * the implicit scheme while option thermal_lookahead is on, and thermal_lookahead = 1 while the scheme is implicit;
 * cetkmc_run_supersteps and cetkmc_run_supersteps_local while the scheme is implicit (Mode B is out of scope). */
enum { CETKMC_THERMAL_EXPLICIT = 0, CETKMC_THERMAL_IMPLICIT = 1 };
struct cetkmc_implicit_info { int64_t updates, steps, launches, coeff_uploads; };
int cetkmc_set_thermal_scheme(void* handle, int scheme);
int cetkmc_ensemble_set_thermal_scheme(void* handle, int scheme);
int cetkmc_get_implicit_info(void* handle, struct cetkmc_implicit_info* info);
int cetkmc_implicit_coeffs(int L, double r, double* inv, double* p);

/* ---- thermal boundary conditions of the implicit scheme ----------------------------------------------
 * Opt-in; with no boundary set (or every beta 0) every update is section 26's, launch for launch.  Six faces, in the order of the
 * enum: i_lo is the substrate side, i_hi the top (plane L - 1).  Face f carries beta[f] >= 0, T_ext[f] and ramp[f]; the voxel on
 * the face sees a ghost node of value x + beta * (T_f - x): beta = 0 adiabatic, 1 a fixed temperature at the ghost node,
 * h dx / k a convective face, any finite beta >= 0 allowed.  One implicit step is section 26's with the 1-D operator of an
 * axis with faces (lo, hi) changed at its two ends only:
 *   diagonal     row 0: 1 + r (1 + beta_lo), row L - 1: 1 + r (1 + beta_hi), L = 1: 1 + r (beta_lo + beta_hi); inside 1 + 2 r;
 *   coefficients inv[0] = 1 / diag_0, p[0] = r inv[0], inv[m] = 1 / (diag_m - r p[m - 1]), p[m] = r inv[m]
 *                (cetkmc_implicit_coeffs_bc; both beta 0: the bits of cetkmc_implicit_coeffs);
 *   right side   c_f = (r * beta_f) * T_f, in double on the host; y[0] = (b[0] + c_lo) inv[0], and for L > 1
 *                y[L - 1] = ((b[L - 1] + c_hi) + r y[L - 2]) inv[L - 1]; L = 1: ((b + c_lo) + c_hi) inv[0].  An addend is applied
 *                only where beta_f != 0: an adiabatic face keeps section 26's arithmetic, -0.0 included.
 * The face temperature of an update: T_f = T_ext[f] + ramp[f] * (double)u, u = g / 20 for the update a stepping call makes at
 * global step g (independent of how a run is cut into calls), u = 0 for a direct update and for cetkmc_time_thermal.  T_f is
 * not clipped.  thermal_substeps = n: n steps with the r of dt / n and the same T_f.  Remelting follows the update as before.
 *   cetkmc_set_thermal_boundary            a single handle; NULL = adiabatic.  Invalidates nothing, leaves the applied-update marker
 *   cetkmc_ensemble_set_thermal_boundary   an ensemble handle: one boundary for all replicas
 *   cetkmc_get_thermal_boundary            the boundary as set (b) and running totals (info) of the updates made with a
 *                      non-adiabatic boundary: updates, their steps, their launches (three per step: the boundary
 *                      instantiations of k_imp_rows, k_imp_lines<1>, k_imp_lines<0>) and rebuilds of the device's [3][2][L] table (one per change of r or
 *                      of a beta; a changed T_ext or ramp travels in the launch).  Either pointer may be NULL.
 *                      cetkmc_get_implicit_info goes on counting every implicit update.
 *   cetkmc_implicit_coeffs_bc              the host routine behind the table; needs no device
 * Refused, before anything is allocated or launched: a negative or non-finite beta; a non-finite T_ext or ramp; a non-adiabatic
 * boundary while the scheme is explicit, and the explicit scheme while a non-adiabatic boundary is set; the per-handle setter on
 * an ensemble's handle or on its replicas; a stepping call one of whose own updates would have a non-finite T_f on a face with
 * beta != 0; cetkmc_implicit_coeffs_bc with L < 1, a non-finite or negative r or beta. */
enum { CETKMC_FACE_I_LO = 0, CETKMC_FACE_I_HI, CETKMC_FACE_J_LO, CETKMC_FACE_J_HI, CETKMC_FACE_K_LO, CETKMC_FACE_K_HI };
struct cetkmc_thermal_boundary { double beta[6], T_ext[6], ramp[6]; };
struct cetkmc_boundary_info { int64_t updates, steps, launches, coeff_uploads; };
int cetkmc_set_thermal_boundary(void* handle, const struct cetkmc_thermal_boundary* b);
int cetkmc_ensemble_set_thermal_boundary(void* handle, const struct cetkmc_thermal_boundary* b);
int cetkmc_get_thermal_boundary(void* handle, struct cetkmc_thermal_boundary* b, struct cetkmc_boundary_info* info);
int cetkmc_implicit_coeffs_bc(int L, double r, double beta_lo, double beta_hi, double* inv, double* p);

/* ---- beam tables: laser scan paths and a volumetric source, built on the device -----------------------
 * Opt-in; with no beam set every kernel, launch, counter and byte is what it was.  A Gaussian beam is separable, so the source of a
 * laser-mode update need not cross to the device as an L * L plane: a beam table holds, for the update ordinals u0 .. u0 + n_u - 1
 * (u = g / 20 for the update a stepping call makes at global step g), one row of factors each, and a depth profile:
 *   amp[n_u], gj[n_u][L], gk[n_u][L], fi[depth], all finite and >= 0, 1 <= depth <= L.
 * The source of update u is row x = u - u0.  Voxel (i, j, k) at depth d = L - 1 - i receives
 *   qv    = d < depth ? (amp[x] * fi[d]) * (gj[x][j] * gk[x][k]) : 0.0        three multiplies in this order, no contraction
 *   qterm = qv != 0.0 ? qv / rho_cp : 0.0
 * and everything else is the implicit step of section 26 (with the boundary of section 27 when one is set): scrub, b = T + dt *
 * (qterm + latent_coef * dF), the solves along k, j, i, the clip, prev_state := state, thermal_substeps = n steps of dt / n from
 * the same row, the melt pass behind the update.  With depth 1 and fi = {1.0} an update equals section 26's from the plane
 * q[j][k] = (amp[x] * 1.0) * (gj[x][j] * gk[x][k]) in every bit.  The device forms the products (the beam instantiations of
 * k_imp_rows); no plane is built, copied or stored.
 *   cetkmc_set_beam            a single handle: copies the table to the device (the caller's arrays are free after the return);
 *                              NULL removes the beam.  Invalidates nothing, leaves the applied-update marker alone.
 *   cetkmc_ensemble_set_beam   an ensemble handle: n_sets tables that share u0, n_u and depth; replica r reads set set_of[r]
 *                              (set_of NULL: set r, and n_sets must equal R).  sets NULL removes the beam.
 *   cetkmc_get_beam_info       running totals of the updates made from a table: updates, their steps, their launches (three per
 *                              step), and the tables copied to the device.  An ensemble handle: of cetkmc_run_ensemble's updates.
 *   cetkmc_thermal_beam        one update now from row u - u0: the twin of cetkmc_thermal_laser.  u is the update ordinal in every
 *                              respect: a thermal boundary's face temperatures are those of u as well.
 * While a beam is set, a stepping call with thermal_mode 2 (cetkmc_run_steps, cetkmc_stage_inputs, cetkmc_run_ensemble) takes every
 * update's source from the row of its global ordinal g / 20: q_planes must be NULL and n_q 0; q_used counts as before.  A call
 * that continues a batch stopped with status 2 on an update step needs nothing supplied again.  cetkmc_time_thermal(laser != 0)
 * reads row 0 (update ordinal u0).  thermal_mode 1 updates have no source, with or without a beam.
 * Refused, before anything is allocated or launched, each naming its entry point: n_u < 1; depth outside 1..L; a null array; a
 * negative or non-finite value; a beam while the scheme is explicit, and the explicit scheme while a beam is set; the per-handle
 * setter on an ensemble's handle or on its replicas; sets that differ in u0, n_u or depth; a set_of entry outside [0, n_sets); a
 * stepping call with a beam and a non-null q_planes or a non-zero n_q; a stepping call, or cetkmc_thermal_beam, one of whose own
 * updates falls outside [u0, u0 + n_u) (computed from step0 and n_steps); cetkmc_thermal_laser while a beam is set. */
struct cetkmc_beam {
    int64_t u0;
    int32_t n_u, depth;
    const double *amp, *gj, *gk, *fi;
};
struct cetkmc_beam_info { int64_t updates, steps, launches, table_uploads; };
int cetkmc_set_beam(void* handle, const struct cetkmc_beam* beam);
int cetkmc_ensemble_set_beam(void* handle, int n_sets, const struct cetkmc_beam* sets, const int32_t* set_of);
int cetkmc_get_beam_info(void* handle, struct cetkmc_beam_info* info);
int cetkmc_thermal_beam(void* handle, double dt, int64_t u, int use_latent, int scrub_nan);

/* The lattice shifted on the device (not in the reference): a layer recoated, a frame that follows the beam.
 * No field crosses to the host: bytes_h2d + bytes_d2h of cetkmc_counters grow by at most 256 per lattice.
 * For every voxel v of the new lattice let s = v - d.
 *   s inside [0, L)^3: state, defect mask, theta, phi and T at v take the old values at s, bit for bit (NaN payloads, -0.0).
 *   s outside:         v is exposed: state = fill_state, mask 0, theta = fill_theta, phi = fill_phi, and T = fill_T under
 *                      CETKMC_SHIFT_T_VALUE, the old T at s clamped per axis to [0, L - 1] under CETKMC_SHIFT_T_EDGE.
 * A component |d[a]| >= L exposes everything.  info: exposed = the exposed voxels, kept = L^3 - exposed, dropped[x] = the old
 * voxels of state x whose v + d lies outside, calls = the shifts made on this lattice so far.
 * d = (0, 0, 0) is a no-op: nothing is written, nothing goes stale, calls is unchanged, kept = L^3 and the other counts 0.
 * Any other d leaves the handle exactly as cetkmc_upload of all five new fields would: prev_state := state, row flags cleared,
 * class bytes, interface flags, list and grid and the unit vectors rebuilt, cause "upload_T_or_state" of cetkmc_invalidates
 * raised, a frozen replica unfrozen.  What an upload leaves alone it leaves alone: a staged batch, the nucleation count,
 * cetkmc_counters' step counts, the row-sum parity, every option and thermal setting.
 * The maps move with the lattice.  Solidification map: stamps (exposed: -1) and the five doubles (exposed: +0.0) move, the
 * snapshot becomes the new state and T, so a cetkmc_solid_update right behind reports n_new = n_cleared = 0.  Origin map: the
 * words move (exposed: 0), the census rows move along axis 0 by d[0] with zero fill, cetkmc_origin_seq is unchanged.
 * Ordered behind the handle's pending work on its stream; returns synchronised.
 *   cetkmc_shift            one lattice: a single-slab, single-process handle or a replica handle.
 *   cetkmc_ensemble_shift   an ensemble handle: s[R], one record per replica (d = 0 leaves that replica untouched), info[R] or NULL;
 *                           one launch sequence, one synchronisation and one copy of the counts whatever R.
 * Refused, before anything is allocated or launched, each naming its entry point: a NULL s; fill_state outside 0..4; an unknown
 * T_mode; a non-zero pad; handles with several slabs and rank handles; a single-lattice handle given to the ensemble call.
 * Non-finite fill values are allowed, as the lattice admits them. */
enum { CETKMC_SHIFT_T_VALUE = 0, CETKMC_SHIFT_T_EDGE = 1 };
struct cetkmc_shift {            /* 48 bytes */
    int32_t d[3];                /* voxel v = (i, j, k) of the old lattice moves to v + d */
    int32_t fill_state;          /* 0..4: state of the exposed voxels */
    int32_t T_mode;              /* CETKMC_SHIFT_T_VALUE or _EDGE */
    int32_t pad;                 /* 0 */
    double  fill_T, fill_theta, fill_phi;
};
struct cetkmc_shift_info {       /* 72 bytes; this call's counts, and calls = running total on the handle */
    int64_t calls, kept, exposed;
    int64_t dropped[6];          /* old voxels that left the lattice, by old state 0..4, [5] = other */
};
int cetkmc_shift(void* handle, const struct cetkmc_shift* s, struct cetkmc_shift_info* info /* may be NULL */);
int cetkmc_ensemble_shift(void* handle, const struct cetkmc_shift* s /* [R] */, struct cetkmc_shift_info* info /* [R] or NULL */);
/* Measurement helper (tools/shift_timing.py): cetkmc_shift -- or, on an ensemble's handle, cetkmc_ensemble_shift with s[R] and
 * info[R] -- between two hipEvents on the handle's stream; *ms = the time between them, from the first launch to the end of
 * the call's last copy.  The shift is real. */
int cetkmc_time_shift(void* handle, const struct cetkmc_shift* s, struct cetkmc_shift_info* info /* may be NULL */, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* CETKMC_H */
