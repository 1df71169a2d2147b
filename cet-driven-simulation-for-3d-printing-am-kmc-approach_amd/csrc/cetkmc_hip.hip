// cetkmc_hip.hip -- C ABI (include/cetkmc.h) + host orchestration of the HIP kernels.
//
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off
//        -fno-fast-math cetkmc_hip.hip -o libcetkmc_hip.so -ldl
// RCCL is dlopen()ed lazily (only multi-process runs need it).  There is no CPU fallback:
// every compute entry point fails if no HIP device is usable.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <climits>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.hpp"
#include "cluster.hpp"
#include "superstep.hpp"
#include "local.hpp"
#include "ensemble.hpp"
#include "front.hpp"
#include "layer.hpp"
#include "texture.hpp"
#include "grain.hpp"
#include "solid.hpp"
#include "origin.hpp"
#include "melt.hpp"
#include "thermal_sub.hpp"
#include "thermal_imp.hpp"
#include "shift.hpp"

using namespace cetkmc;

namespace {

thread_local std::string g_err;
int fail(const std::string& m) { g_err = m; return 1; }

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + \
                        ":" + std::to_string(__LINE__) + ")");                              \
    } while (0)
#define CHK(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

int next_pow2(int n) { int p = 1; while (p < n) p <<= 1; return p; }
int round_up(int n, int m) { return (n + m - 1) / m * m; }

// ---- kernel launches ------------------------------------------------------------------
// One launch.  With ev_a and ev_b the two hipEvents ride on the dispatch itself (hipExtLaunchKernelGGL start / stop events =
// the dispatch's own begin / end timestamps: no barrier packets in the stream, so a timed launch runs like an untimed
// one); without them it is a plain launch.  The arguments are converted to the kernel's own parameter types.
template <class T> struct arg_of { using type = T; };
template <class... P>
void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t shmem, hipStream_t st, hipEvent_t ev_a, hipEvent_t ev_b,
            typename arg_of<P>::type... args)
{
    if (ev_a && ev_b) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)shmem, st, ev_a, ev_b, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, shmem, st, args...);
}

// Run-time flags -> template arguments: f is called once, with std::true_type / std::false_type values, for exactly the
// combinations the kernels are built for.  with_source: (LASER, LATENT) of the temperature tiles.  with_boundary: the ImpBc that
// leads the trailing pack of the implicit kernels' boundary form, or nothing.
using Yes = std::true_type;
using No = std::false_type;
template <class F> void with_flag(bool on, F&& f) { if (on) f(Yes{}); else f(No{}); }
template <class F> void with_source(int laser, int latent, F&& f) { if (laser && latent) f(Yes{}, Yes{}); else if (laser) f(Yes{}, No{}); else f(No{}, No{}); }
template <class F> void with_boundary(bool on, const ImpBc& B, F&& f) { if (on) f(B); else f(); }
template <class F> void with_beam(bool on, const ImpBeam& M, F&& f) { if (on) f(M); else f(); }

// 20-step temperature updates (kmc_simulation.py:248) among the global steps [step0, step0 + n): multiples of 20 below
// step0 + n less those below step0
int64_t updates_in(int64_t step0, int64_t n)
{
    auto below = [](int64_t x) { return (x > 0 ? x + 19 : x) / 20; };       // ceil(x / 20)
    return n > 0 ? below(step0 + n) - below(step0) : 0;
}

// ---- RCCL, loaded on demand -----------------------------------------------------------
struct Rccl {
    void* so = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
} g_rccl;

int load_rccl()
{
    if (g_rccl.so) return 0;
    const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void* so = nullptr;
    for (const char* n : names) if ((so = dlopen(n, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!so) return fail(std::string("cannot load librccl.so: ") + dlerror());
#define SYM(field, name)                                                         \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(so, name));    \
    if (!g_rccl.field) return fail(std::string("librccl.so lacks ") + name);
    SYM(GetUniqueId, "ncclGetUniqueId")
    SYM(CommInitRank, "ncclCommInitRank")
    SYM(CommDestroy, "ncclCommDestroy")
    SYM(AllGather, "ncclAllGather")
    SYM(Send, "ncclSend")
    SYM(Recv, "ncclRecv")
    SYM(GroupStart, "ncclGroupStart")
    SYM(GroupEnd, "ncclGroupEnd")
    SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
    g_rccl.so = so;
    return 0;
}
#define NCCLCHK(expr)                                                                             \
    do {                                                                                          \
        ncclResult_t r_ = (expr);                                                                 \
        if (r_ != ncclSuccess)                                                                    \
            return fail(std::string(#expr) + ": " + g_rccl.GetErrorString(r_));                   \
    } while (0)

// ---- handle ---------------------------------------------------------------------------
// A beam table on the device as the settings name it; the memory belongs to the handle or the ensemble
// that was given the table (Handle::d_beam, Ens::d_beam).  One set is set_stride doubles: amp[n_u], gj[n_u][L], gk[n_u][L],
// fi[depth].  base: where the set of this handle begins (a replica: set_of[r] * set_stride); set_of: the ensemble's device
// array [R], read by the ensemble's own launches alone.
struct BeamView {
    bool on = false;
    const double* d = nullptr;
    const int32_t* set_of = nullptr;
    int64_t u0 = 0, set_stride = 0, base = 0;
    int n_u = 0, depth = 0, L = 0;
};
// How temperature updates are made (DESIGN.md sections 24 to 28), as the setters leave it.  A handle holds one; an ensemble holds
// one for all its replicas and hands it to each (share_thermal), so a direct update on a replica handle follows the ensemble.
struct ThermalSettings {
    int substeps = 1;                    // n: every update is n steps of dt / n (thermal_sub.hpp)
    int scheme = CETKMC_THERMAL_EXPLICIT;        // or _IMPLICIT (thermal_imp.hpp)
    cetkmc_thermal_boundary bc{};        // as set; every beta 0: adiabatic, the launches and the table of section 26
    bool bc_on = false;                  // some beta != 0
    int remelt_on = 0;                   // the stepping loop melts behind every temperature update (melt.hpp)
    double remelt_threshold = 0.0;
    BeamView beam{};                     // on: the source of every laser-mode update is a row of this table, not a plane
};
// what the updates made so far add up to: a handle's by its own calls, an ensemble's by cetkmc_run_ensemble
struct ThermalInfo { cetkmc_substep_info sub{}; cetkmc_implicit_info imp{}; cetkmc_boundary_info bc{}; cetkmc_beam_info beam{}; };
// A device table of Thomas coefficients and what it was built for (compared by bits): [2][L], inv and p of r (section 26), or
// [3][2][L], inv and p per axis of r and the six beta (section 27).  Allocated by the first update that reads it.
struct CoefTable { double* d = nullptr; double r = 0.0, beta[6] = {}; };

struct Slab {
    SlabView v{};
    uint8_t* prev = nullptr;
    double* Tbuf[2] = {nullptr, nullptr};
    double* vvalbuf[2] = {nullptr, nullptr};     // rate table of Tbuf[b] (the pair is flipped together)
    double* depbuf[2] = {nullptr, nullptr};      // plane L-1 deposition rates of Tbuf[b]
    double* rowsumbuf[2] = {nullptr, nullptr};   // the two row-sum pairs (one allocation each: the sums, then the counts);
    int32_t* rowcntbuf[2] = {nullptr, nullptr};  // v.rowsum / v.rowcnt are the pair Handle::row_par names
    size_t nR = 0;                               // bytes of a pair
    size_t nS = 0, nT = 0, nC = 0;   // bytes of a u8 array, doubles of an f64 array, bytes of the class array
};

struct Handle {
    cetkmc_params p{};
    KParams kp{};
    int L = 0, Pk = 1, PB = 1, RJ = 0, pitchS = 0, pitchT = 0, pitchC = 0;
    int dev = 0;
    hipStream_t stream = nullptr, stream2 = nullptr;
    std::vector<Slab> slabs;
    SlabView* d_views[4] = {nullptr, nullptr, nullptr, nullptr};   // [T-buffer parity + 2 * row-sum parity]
    int cur = 0;                                 // current T buffer
    int row_par = 0;                             // current row-sum pair: the one every slab's v.rowsum / v.rowcnt point to, so
                                                 // whatever takes a view (view_of, dviews) reads and writes the current pair
    int G = 1, my_first = 0;                     // global slab count, index of first local slab
    int own_i0 = 0, own_i1 = 0;
    BlockEnt* d_blocks = nullptr;
    cetkmc_event* d_events_all = nullptr;
    StepState* d_ss = nullptr;
    int* d_dirty = nullptr;      // [1 + DIRTY_MAX] rows made stale by the last applied event (incremental mode)
    PendRec* d_pend = nullptr;   // the event of a deferred step, applied by the next sweep launch (k_select_pend -> k_sweep_stream_apply)
    int apply_in_sweep = 1;      // option "apply_in_sweep": defer the application of eligible batched steps into the next sweep
    int fused_tiles = 1;         // option "fused_tiles": 1 = the sweep launch that applies a pending event runs census-free tiles
                                 // (sweep_table_tile) at 128 < L <= 256, 2 = the plain launch at that shape as well, 0 = ring tiles
    int table_lane_skip = 1;     // option "table_lane_skip": 1 = those tiles request the class bytes first and the table entries only in
                                 // the lanes that can use them (lane_needs_values()), 0 = every lane's entries; same bits
    int lane_sums = 1;           // option "lane_sums": 1 = the skipping tiles of the deferred launches request the 8 B lane sum of a pristine
                                 // chunk instead of its 64 B of entries while the lane table is fresh (kernels.hpp, "lane sums"); 0 = entries
    int early_tiles = -1;        // option "early_tiles": tiles of the next step's sweep that a deferred step's selection launch runs
                                 // (k_select_pend_tiles, into the other row-sum pair); 0 = k_select_pend and one pair; -1 (default) =
                                 // a quarter of the tile range, 1024 of 4096 at 256^3, where it was measured
    int early_blocks = 256;      // option "early_blocks": tile blocks of that launch (each takes several tiles in turn: one block per
                                 // CU, four tiles each at 256^3); 0 = one per tile
    int poison_alt_rows = 0;     // option "poison_alt_rows" (tests): the pair about to be written is filled with 0xFF first
    bool pend_live = false;      // run_steps: the next launch_sweep applies *d_pend (the previous step was deferred)
    int lane_build = 1;          // option "lane_build": 1 = the temperature tiles that write the rate table store the lane table too
                                 // (k_thermal_tiles16<.., LANES>: the plain launch behind the update does not build), 0 = that launch builds
    int lane_sweep = 1;          // option "lane_sweep": 1 = a plain sweep launch reads lane sums while the lane table is fresh
                                 // (k_sweep_stream<.., LU>), 0 = the plain launch reads every entry
    int64_t cnt_lane_builds = 0; // plain launches that built the lane table (cetkmc_lane_table)
    int64_t cnt_lane_builds_thermal = 0;   // temperature updates whose tiles built it
    int pend_early = 0;          // ... and leaves out its first pend_early tiles, which the selection launch ran
    BatchCfg pend_cfg{};         // ... with this batch configuration
    double* d_ktab = nullptr;
    KParams* d_kp = nullptr;
    void* d_scratch = nullptr;
    size_t scratch_bytes = 0;
    int* d_flag = nullptr;
    double* d_qtop = nullptr;
    // batch buffers
    double *d_u_pick = nullptr, *d_u_defect = nullptr, *d_u_np = nullptr, *d_q = nullptr, *d_log_total = nullptr;
    cetkmc_event* d_log_event = nullptr;
    int64_t* d_log_nev = nullptr;
    size_t cap_steps = 0, cap_np = 0, cap_q = 0;
    // page-locked host staging for a batch's inputs and logs: copies to / from it are queued on the stream like kernels
    // (a copy to or from pageable memory blocks the caller once per array)
    char* pin_in = nullptr; size_t pin_in_cap = 0;
    char* pin_out = nullptr; size_t pin_out_cap = 0;
    // a batch whose host inputs are already in d_u_pick / d_u_defect / d_u_np / d_q (cetkmc_stage_inputs)
    struct { bool valid = false, has_defect = false; int64_t step0 = 0, n_steps = 0, np_cap = 0, n_q = 0; int thermal_mode = 0; } staged;
    // rccl
    ncclComm_t comm = nullptr;
    int rank = 0, nranks = 1;
    bool swept = false;
    int sweep_auto = 1;        // sweep_variant never set explicitly: lattices of L <= 128 take variant 4 (launch-bound there: one launch
                               // less per sweep; same bits), larger ones variant 1
    int sweep_variant = 1;     // 0 simple, 1 streaming + rate table with the LDS census (default), 2 streaming, nucleation rates
                               // recomputed per sweep, 3 census-free table sweep (same bits, measured no faster: DESIGN.md section 13)
    bool table_fresh = false;  // vval / dep_val match the current T and parameters (k_rate_table)
    bool ifc_fresh = false;    // vval / event count (class byte) of every listed voxel match the current lattice, T, defects and parameters
    bool lanes_fresh = false;  // the lane table (Slab::v.lanesum / lanecnt) was built from the current table and every write of an entry
                               // since then went through ifc_store(); follows TABLE and IFC: whatever clears either clears it
    int ifc_every_step = 0;    // 1: k_interface before every full sweep (round-1 behaviour, A/B); 0: only when stale --
                               // between temperature updates the apply kernel re-evaluates the <= 30 listed voxels an event touches
    int thermal_variant = 1;   // 1 = plane-marching LDS kernel, 0 = one thread per voxel
    int thermal_general = 0;   // 1: k_thermal_march also where k_thermal_tiles applies (A/B, tests)
    int therm_ni = THERM_NI;   // planes per block of the marching kernel
    int therm_ni16 = THERM16_NI;   // planes per block of k_thermal_tiles16
    int thermal_rpt = 2;       // rows per thread of k_thermal_tiles16 (2: 1024 threads per block at 256 columns (default); 4: 512)
    int thermal_kt = 256;      // columns per tile of k_thermal_tiles16 (256, or 128 with 2 rows per thread: 512 threads)
    int thermal_tiles16 = 1;   // 1: the 16-row k_thermal_tiles16 where tiles apply (default); 0: the 8-row k_thermal_tiles (round-2 kernel)
    int ifc_blocks = 64;       // grid of k_interface (grid-stride over the device-side list length)
    int ifc_block = 256;
    size_t shmem_stream = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // grain clustering (cetkmc_cluster): results kept until the next call
    int *d_cc_parent = nullptr, *d_cc_roots = nullptr, *d_cc_cid = nullptr, *d_cc_labels = nullptr, *d_cc_stats = nullptr, *d_cc_n = nullptr;
    int64_t cc_n_clusters = -1;
    std::vector<int> cc_roots_sorted;
    std::vector<hipEvent_t> prof;
    cetkmc_host_comm hc{};       // host-relay transport (cetkmc_create_rank_host); used when comm is null
    // profile 2: every collective of the batch is bracketed by a hipEvent pair on the stream (RCCL: the collective's own
    // device time; host relay: copies + callback + the synchronisations around them)
    bool time_comm = false;
    std::vector<hipEvent_t> comm_ev;
    size_t comm_ev_used = 0;
    std::vector<char> hc_stage;
    cetkmc_counters cnt{};       // cetkmc_get_counters: work issued / bytes moved / per-phase device time
    // look-ahead temperature update: T(n+1) + its rate table computed on stream2 while the 19 steps between two updates run
    struct Spec {
        bool valid = false;
        int64_t g = -1;          // global step of the update it stands for
        int laser = 0, use_latent = 0, scrub = 0;
        double dt = 0.0;
        const double* d_q = nullptr;
    } spec;
    // A batch that stops with status 2 (stream exhausted) ON a temperature-update step has already applied that step's update
    // (the thermal kernels run before the selection notices the shortage).  The continuation batch starts at the same
    // global step: it must not apply the update a second time (kmc_simulation.py:248-250 updates T once per 20 steps).
    int64_t therm_applied_g = -1;
    int thermal_table = 1;       // option "thermal_table": the default temperature tiles write the rate table too (no k_rate_table launch)
    int thermal_ahead = 0;       // option "thermal_lookahead": off by default -- measured slower on one GPU:
                                 // the look-ahead kernels run right behind the update, beside the next sweeps, which they slow down
                                 // by more than the update costs (both are memory bound, and they evict the sweep's working set)
    hipEvent_t ev_main = nullptr, ev_spec = nullptr;
    // cetkmc_run_supersteps' working buffers (grow-only: run_kmc(mode="B") under the event-count thermal clock makes one call
    // per super-step, which five hipMalloc / hipFree pairs per call would dominate)
    cetkmc_event* d_sup_dom = nullptr; size_t cap_sup_dom = 0;
    DomPick* d_sup_picks = nullptr; size_t cap_sup_picks = 0;
    unsigned long long* d_sup_cnt = nullptr; size_t cap_sup_cnt = 0;
    cetkmc_event* d_sup_log = nullptr; size_t cap_sup_log = 0;
    double* d_sup_rmax = nullptr; size_t cap_sup_rmax = 0;
    // cetkmc_run_supersteps_local: per-super-step logs of the horizon and of the capped boxes
    double* d_loc_horizon = nullptr; size_t cap_loc_horizon = 0;
    int64_t* d_loc_capped = nullptr; size_t cap_loc_capped = 0;
    // front statistics and layer profile: block partials and results of the pass issued on this handle, [R] lattices each
    // (grow-only, as above), and the class byte of every grain (offs[r] + r + id)
    FrontPart* d_front_part = nullptr; size_t cap_front_part = 0;
    FrontStats* d_front_out = nullptr; size_t cap_front_out = 0;
    LayerRec* d_layer_part = nullptr; size_t cap_layer_part = 0;
    LayerRec* d_layer_out = nullptr; size_t cap_layer_out = 0;
    uint8_t* d_layer_eq = nullptr; size_t cap_layer_eq = 0;
    bool own_streams = true;     // false: a replica of an ensemble, on the streams of replica 0
    bool ens_member = false;     // replica r >= 1 of an ensemble (released with it)
    bool in_ensemble = false;    // any replica: stepped by cetkmc_run_ensemble only
    int64_t state_uploads = 0;   // lattice (state) uploads so far: a new lattice in a replica unfreezes it
    int64_t shift_calls = 0;     // cetkmc_shift: shifts of this lattice so far (d = 0 is none)
    // solidification map (cetkmc_solid_begin .. _end, solid.hpp): the arrays of this lattice; d_solid_block owns them on a
    // single handle (a replica's lie in its ensemble's block)
    SolidMap solid{};
    void* d_solid_block = nullptr;
    bool solid_on = false;
    int64_t solid_recorded = 0;  // voxels with stamp >= 0
    // origin map (cetkmc_origin_begin .. _end, origin.hpp): words and census of this lattice; d_origin_block owns them on a
    // single handle, the ensemble's block on a replica
    OriginMap origin{};
    void* d_origin_block = nullptr;
    bool origin_on = false;
    int64_t origin_seq = 0;      // ordinal of the next absorbed step
    // remelting (cetkmc_set_remelt / cetkmc_remelt, melt.hpp): row flags and counters of this lattice, allocated when remelting
    // is first used
    MeltState melt{};
    void* d_melt_block = nullptr;
    cetkmc_remelt_info melt_info{};      // the counters as last read (end of a stepping call, end of a direct pass)
    ThermalSettings ts{};        // cetkmc_set_remelt / _thermal_substeps / _thermal_scheme / _thermal_boundary / _beam
    ThermalInfo ti{};
    CoefTable coef{}, coef_bc{}; // of the implicit updates without / with a boundary (two: clearing a boundary uploads nothing)
    double* d_beam = nullptr;    // cetkmc_set_beam: the table ts.beam names
    // sub-stepped temperature updates (thermal_sub.hpp)
    int substep_block = 0;       // option "substep_block": sub-steps per k_thermal_sub launch; 0 = the measured default (SUB_SDEFAULT at
                                 // L > SUB_PLAIN_L, else the plain path), 1 = the plain path (n launches of the existing kernel) on any handle
    int substep_planes = 0;      // option "substep_planes": planes per block of k_thermal_sub; 0 = one round of blocks on the device
    int n_cu = 0;                // compute units of the device (read when first needed)
};

// ---- cache state ------------------------------------------------------------------------------------
// What a handle keeps between calls -- swept (SWEEP), table_fresh (TABLE), ifc_fresh (IFC), therm_applied_g (APPLIED),
// staged.valid (STAGED) -- goes stale HERE and nowhere else: a call site names what happened (a Cause), the table says which
// caches that costs, invalidate() clears them.  A cache becomes fresh where the launch that makes it so is issued
// (ensure_table, launch_sweep, launch_dirty_rows, the temperature tiles that write the table, the look-ahead adoption,
// cetkmc_stage_inputs).  cetkmc_invalidates() exports the table by name.
enum class Cause : int {
    upload, upload_T_or_state, set_params, option_sweep_variant, option_interface_every_step, option_reserve_batch, set_defects,
    set_prev_state_null, set_prev_state_array, apply, thermal_update, thermal_update_wrote_table, lookahead_adopted, step,
    step_no_upkeep, batch_stopped, ensemble_stepped, batch_begin, table_written, marker_taken, count
};
struct CauseRow { Cause cause; const char* name; unsigned stale; };
constexpr unsigned SWEEP = CETKMC_CACHE_SWEEP, TABLE = CETKMC_CACHE_TABLE, IFC = CETKMC_CACHE_IFC, APPLIED = CETKMC_CACHE_APPLIED,
                   STAGED = CETKMC_CACHE_STAGED;
// two rules, each stated once: whoever writes the table overwrites the listed voxels' entries with it (the interface kernel has
// to follow), and a new field -- an upload, a temperature update -- is no longer the one the stopped batch's update produced
constexpr unsigned WROTE_TABLE = IFC, NEW_FIELD = APPLIED;
constexpr CauseRow INVALIDATES[] = {
    // cetkmc_upload / _upload_planes, any field (orientations only and defects only as well: every rate may read them) ...
    {Cause::upload, "upload", SWEEP | IFC | NEW_FIELD},
    // ... with T or state: a new state also changes the interface list, and a voxel that leaves it keeps its interface sum in
    // the table until the table is rewritten
    {Cause::upload_T_or_state, "upload_T_or_state", SWEEP | TABLE | IFC | NEW_FIELD},
    {Cause::set_params, "set_params", SWEEP | TABLE | IFC},
    {Cause::option_sweep_variant, "option_sweep_variant", SWEEP | TABLE | IFC},
    {Cause::option_interface_every_step, "option_interface_every_step", IFC},
    {Cause::option_reserve_batch, "option_reserve_batch", STAGED},        // growing a buffer moves it
    // the defect mask replaced: cetkmc_set_defects, _set_defects_sparse, a replica with counts[r] >= 0 of the ensemble call
    {Cause::set_defects, "set_defects", SWEEP | IFC},
    {Cause::set_prev_state_null, "set_prev_state_null", IFC},             // the interface list is rebuilt in address order
    {Cause::set_prev_state_array, "set_prev_state_array", 0},
    {Cause::apply, "apply", SWEEP | IFC},                                 // the touched voxels' codes are current, their sums are not
    {Cause::thermal_update, "thermal_update", SWEEP | TABLE | NEW_FIELD},
    {Cause::thermal_update_wrote_table, "thermal_update_wrote_table", SWEEP | WROTE_TABLE | NEW_FIELD},
    // the field a batch computed ahead (with its table) becomes the current one.  No NEW_FIELD: a look-ahead is
    // launched behind a synchronous update of the same batch, which dropped the marker
    {Cause::lookahead_adopted, "lookahead_adopted", SWEEP | WROTE_TABLE},
    {Cause::step, "step", SWEEP},                                         // a batched step executed (Mode A, Mode B)
    // ... whose apply kernel did not re-evaluate the listed voxels it touched (interface_every_step, sweep_variant 0)
    {Cause::step_no_upkeep, "step_no_upkeep", SWEEP | IFC},
    // A batch stopped early (status != 0): the steps still queued behind the stop ran as pass-throughs (temperature copied
    // through, buffer pair flipped, rate table / interface kernels returning at once), so the host's flags describe work the
    // device skipped.  Both are recomputed from the field as it stands.
    {Cause::batch_stopped, "batch_stopped", SWEEP | TABLE | IFC},
    // a replica stepped by cetkmc_run_ensemble: its flags describe nothing the ensemble kernels maintained
    {Cause::ensemble_stepped, "ensemble_stepped", SWEEP | TABLE | IFC | NEW_FIELD},
    // a stepping call begins (cetkmc_run_steps, _run_supersteps, _stage_inputs): a staged batch is consumed or dropped, the
    // batch buffers are reused
    {Cause::batch_begin, "batch_begin", STAGED},
    {Cause::table_written, "table_written", WROTE_TABLE},                 // ensure_table
    {Cause::marker_taken, "marker_taken", APPLIED},                       // cetkmc_run_steps hands the marker to its batch
};
constexpr int N_CAUSES = (int)Cause::count;
constexpr bool causes_in_order()
{
    for (int c = 0; c < N_CAUSES; ++c) if ((int)INVALIDATES[c].cause != c) return false;
    return true;
}
static_assert(sizeof INVALIDATES / sizeof *INVALIDATES == N_CAUSES && causes_in_order(), "INVALIDATES[]: one row per Cause, in its order");

void invalidate(Handle* h, Cause c)
{
    const unsigned stale = INVALIDATES[(int)c].stale;
    if (stale & SWEEP) h->swept = false;
    if (stale & TABLE) h->table_fresh = false;
    if (stale & IFC) h->ifc_fresh = false;
    // the lane table is a digest of the rate table and of the class bytes as the batched apply keeps them: every cause that
    // rewrites the table, leaves listed voxels' entries to be rewritten or changes the lattice outside the batched apply
    // carries TABLE or IFC
    if (stale & (TABLE | IFC)) h->lanes_fresh = false;
    if (stale & APPLIED) h->therm_applied_g = -1;
    if (stale & STAGED) h->staged.valid = false;
}

KParams make_kparams(const cetkmc_params& p)
{
    KParams k{};
    k.nu = p.nu; k.nu_dep = p.nu_dep;
    for (int a = 0; a < 3; ++a) { k.E_b[a] = p.E_b[a]; k.E_diff[a] = p.E_diff[a]; }
    k.kT = p.kT; k.T_melt = p.T_melt; k.I0 = p.I0; k.delta_T_c = p.delta_T_c;
    k.rate_threshold = p.rate_threshold; k.anisotropy = p.anisotropy;
    k.impurity_re = p.impurity_re; k.impurity_c = p.impurity_c;
    k.K_nuc = p.K_nuc; k.beta_imp_nuc = p.beta_imp_nuc; k.max_imp_frac = p.max_imp_frac;
    return k;
}

// kmc_event_rates.py:126-128, same expression order as the device helper k_eff()
double host_k_eff(const cetkmc_params& p, int n_nb, int n_imp)
{
    int den = n_nb > 1 ? n_nb : 1;
    double x = (double)n_imp / (double)den;
    double f_imp = (x < p.max_imp_frac) ? x : p.max_imp_frac;
    double K = p.K_nuc * (1.0 - p.beta_imp_nuc * f_imp);
    double m = (K < p.K_nuc) ? K : p.K_nuc;
    double lo = 0.1 * p.K_nuc;
    return (m > lo) ? m : lo;
}

int upload_ktab(Handle* h)
{
    double tab[225];
    for (int a = 0; a < 15; ++a)
        for (int b = 0; b < 15; ++b) tab[a * 15 + b] = host_k_eff(h->p, a, b);
    HIPCHK(hipMemcpyAsync(h->d_ktab, tab, sizeof tab, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->d_kp, &h->kp, sizeof(KParams), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int push_views(Handle* h)
{
    for (int par = 0; par < 4; ++par) {
        std::vector<SlabView> v;
        for (auto& s : h->slabs) {
            SlabView x = s.v;
            x.T = s.Tbuf[par & 1]; x.vval = s.vvalbuf[par & 1]; x.dep_val = s.depbuf[par & 1];
            x.rowsum = s.rowsumbuf[par >> 1]; x.rowcnt = s.rowcntbuf[par >> 1];
            v.push_back(x);
        }
        HIPCHK(hipMemcpyAsync(h->d_views[par], v.data(), v.size() * sizeof(SlabView), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int ensure_scratch(Handle* h, size_t bytes)
{
    if (bytes <= h->scratch_bytes) return 0;
    if (h->d_scratch) HIPCHK(hipFree(h->d_scratch));
    h->d_scratch = nullptr; h->scratch_bytes = 0;
    HIPCHK(hipMalloc(&h->d_scratch, bytes));
    h->scratch_bytes = bytes;
    return 0;
}

int create_common(const cetkmc_params* p, int L, const std::vector<std::pair<int, int>>& ranges, int dev,
                  int G, int my_first, void** out, const Handle* share = nullptr)
{
    if (!p || !out) return fail("null argument");
    if (L < 1) return fail("L must be >= 1");
    if (3 * L > PMAX) return fail("L too large for this build (3L <= " + std::to_string(PMAX) + ")");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail("no usable HIP device: libcetkmc_hip has no CPU fallback");
    if (dev < 0 || dev >= ndev) return fail("device id out of range");
    HIPCHK(hipSetDevice(dev));
    Handle* h = new Handle();
    h->p = *p; h->kp = make_kparams(*p);
    h->L = L; h->Pk = next_pow2(L); h->PB = next_pow2(3 * L);
    h->RJ = round_up(L, SWEEP_TJ) + 4;
    h->pitchS = round_up(KOFF + L + 4, 16);
    h->pitchT = round_up(L, 8);      // rows of the f64 fields are 64-B multiples: a sweep lane reads 8 entries unconditionally
    if (const char* e = getenv("CETKMC_IFC_BLOCK")) h->ifc_block = atoi(e);
    h->pitchC = round_up(KOFFC + L + 12, 16);
    h->shmem_stream = (size_t)STREAM_SLOTS * (SWEEP_TJ + 4) * h->pitchC;
    if (h->shmem_stream > 64 * 1024 || (SWEEP_TJ + 4) * h->pitchC > 16 * 256 * STREAM_MAXPF) { delete h; return fail("L too large for the LDS ring"); }
    h->dev = dev; h->G = G; h->my_first = my_first;
    if (share) {     // a replica of an ensemble: every replica's work is ordered on one stream
        h->stream = share->stream; h->stream2 = share->stream2; h->own_streams = false;
    } else {   // the stepping loop's stream at the highest priority, the look-ahead stream at the lowest: its workgroups are
        // dispatched into what the main stream leaves free (the one-block selection kernels leave almost everything)
        int least = 0, greatest = 0;
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, greatest));
        HIPCHK(hipStreamCreateWithPriority(&h->stream2, hipStreamNonBlocking, least));
    }
    HIPCHK(hipEventCreate(&h->ev0));
    HIPCHK(hipEventCreate(&h->ev1));
    HIPCHK(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&h->ev_spec, hipEventDisableTiming));
    h->own_i0 = ranges.front().first;
    h->own_i1 = ranges.back().first + ranges.back().second;
    for (auto& r : ranges) {
        Slab s;
        s.v.L = L; s.v.gi0 = r.first; s.v.nloc = r.second;
        s.v.RJ = h->RJ; s.v.pitchS = h->pitchS; s.v.pitchT = h->pitchT; s.v.Pk = h->Pk; s.v.pitchC = h->pitchC;
        s.nS = (size_t)(r.second + 4) * h->RJ * h->pitchS;
        s.nT = (size_t)(r.second + 4) * L * h->pitchT;
        s.nC = (size_t)(r.second + 4) * h->RJ * h->pitchC;
        HIPCHK(hipMalloc((void**)&s.v.cls, s.nC));
        HIPCHK(hipMemsetAsync(s.v.cls, 0, s.nC, h->stream));
        HIPCHK(hipMalloc((void**)&s.v.state, s.nS));
        HIPCHK(hipMalloc((void**)&s.v.defects, s.nS));
        HIPCHK(hipMalloc((void**)&s.prev, s.nS));
        HIPCHK(hipMalloc((void**)&s.v.row_chg, (size_t)(s.v.nloc + 4) * L));
        HIPCHK(hipMemsetAsync(s.v.row_chg, 1, (size_t)(s.v.nloc + 4) * L, h->stream));
        HIPCHK(hipMemsetAsync(s.v.state, OOB, s.nS, h->stream));
        HIPCHK(hipMemsetAsync(s.v.defects, 0, s.nS, h->stream));
        HIPCHK(hipMemsetAsync(s.prev, OOB, s.nS, h->stream));
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipMalloc((void**)&s.Tbuf[b], s.nT * sizeof(double)));
            HIPCHK(hipMemsetAsync(s.Tbuf[b], 0, s.nT * sizeof(double), h->stream));
        }
        s.v.T = s.Tbuf[0];
        HIPCHK(hipMalloc((void**)&s.v.theta, s.nT * sizeof(double)));
        HIPCHK(hipMalloc((void**)&s.v.phi, s.nT * sizeof(double)));
        HIPCHK(hipMemsetAsync(s.v.theta, 0, s.nT * sizeof(double), h->stream));
        HIPCHK(hipMemsetAsync(s.v.phi, 0, s.nT * sizeof(double), h->stream));
        HIPCHK(hipMalloc((void**)&s.v.ovec, 3 * s.nT * sizeof(double)));
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipMalloc((void**)&s.vvalbuf[b], s.nT * sizeof(double)));
            HIPCHK(hipMemsetAsync(s.vvalbuf[b], 0, s.nT * sizeof(double), h->stream));
            HIPCHK(hipMalloc((void**)&s.depbuf[b], (size_t)L * h->pitchT * sizeof(double)));
            HIPCHK(hipMemsetAsync(s.depbuf[b], 0, (size_t)L * h->pitchT * sizeof(double), h->stream));
        }
        s.v.vval = s.vvalbuf[0]; s.v.dep_val = s.depbuf[0];
        if (ranges.size() == 1 && L > 128 && h->Pk <= 256) {      // the shape of table_tiles(): one copy, the table's indexing / 8
            HIPCHK(hipMalloc((void**)&s.v.lanesum, s.nT / 8 * sizeof(double)));
            HIPCHK(hipMalloc((void**)&s.v.lanecnt, s.nT / 8));
            HIPCHK(hipMemsetAsync(s.v.lanesum, 0, s.nT / 8 * sizeof(double), h->stream));
            HIPCHK(hipMemsetAsync(s.v.lanecnt, (int)LANE_POISON, s.nT / 8, h->stream));
        }
        HIPCHK(hipMalloc((void**)&s.v.ifc_in, s.nT));
        HIPCHK(hipMalloc((void**)&s.v.ifc_code, s.nT * sizeof(uint32_t)));
        HIPCHK(hipMemsetAsync(s.v.ifc_code, 0xFF, s.nT * sizeof(uint32_t), h->stream));
        HIPCHK(hipMalloc((void**)&s.v.ifc_list, (size_t)r.second * L * L * sizeof(uint32_t)));
        HIPCHK(hipMalloc((void**)&s.v.ifc_n, sizeof(int)));
        HIPCHK(hipMemsetAsync(s.v.ifc_in, 0, s.nT, h->stream));
        HIPCHK(hipMemsetAsync(s.v.ifc_n, 0, sizeof(int), h->stream));
        const size_t n_rows = (size_t)r.second * 3 * L;
        s.nR = n_rows * (sizeof(double) + sizeof(int32_t));
        for (int b = 0; b < 2; ++b) {
            HIPCHK(hipMalloc((void**)&s.rowsumbuf[b], s.nR));
            HIPCHK(hipMemsetAsync(s.rowsumbuf[b], 0, s.nR, h->stream));
            s.rowcntbuf[b] = reinterpret_cast<int32_t*>(s.rowsumbuf[b] + n_rows);
        }
        s.v.rowsum = s.rowsumbuf[0]; s.v.rowcnt = s.rowcntbuf[0];
        h->slabs.push_back(s);
    }
    for (int par = 0; par < 4; ++par) HIPCHK(hipMalloc((void**)&h->d_views[par], h->slabs.size() * sizeof(SlabView)));
    HIPCHK(hipMalloc((void**)&h->d_blocks, (size_t)PMAX * sizeof(BlockEnt)));
    HIPCHK(hipMemsetAsync(h->d_blocks, 0, (size_t)PMAX * sizeof(BlockEnt), h->stream));
    HIPCHK(hipMalloc((void**)&h->d_events_all, (size_t)G * sizeof(cetkmc_event)));
    HIPCHK(hipMemsetAsync(h->d_events_all, 0xFF, (size_t)G * sizeof(cetkmc_event), h->stream));   // type = -1
    HIPCHK(hipMalloc((void**)&h->d_ss, sizeof(StepState)));
    HIPCHK(hipMemsetAsync(h->d_ss, 0, sizeof(StepState), h->stream));
    HIPCHK(hipMalloc((void**)&h->d_dirty, (1 + 2 * DIRTY_MAX) * sizeof(int)));     // list + per-plane arrival counters
    HIPCHK(hipMemsetAsync(h->d_dirty, 0, (1 + 2 * DIRTY_MAX) * sizeof(int), h->stream));
    HIPCHK(hipMalloc((void**)&h->d_pend, sizeof(PendRec)));
    HIPCHK(hipMemsetAsync(h->d_pend, 0, sizeof(PendRec), h->stream));
    HIPCHK(hipMalloc((void**)&h->d_ktab, 225 * sizeof(double)));
    HIPCHK(hipMalloc((void**)&h->d_kp, sizeof(KParams)));
    HIPCHK(hipMalloc((void**)&h->d_flag, sizeof(int)));
    HIPCHK(hipMalloc((void**)&h->d_qtop, (size_t)L * L * sizeof(double)));
    HIPCHK(hipMemset(h->d_qtop, 0, (size_t)L * L * sizeof(double)));      // cetkmc_time_thermal before any cetkmc_thermal_laser
    CHK(upload_ktab(h));
    CHK(push_views(h));
    for (auto& s : h->slabs) hipLaunchKernelGGL(k_orient, dim3(1024), dim3(256), 0, h->stream, s.v);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    *out = h;
    return 0;
}

// the device views of the current T buffer and the current row-sum pair
SlabView* dviews(const Handle* h) { return h->d_views[h->cur + 2 * h->row_par]; }
// The other row-sum pair becomes the current one (a deferred step whose selection launch has run early tiles into it).  Host
// state only: every launch issued from here on takes its views after the flip.
void flip_rows(Handle* h)
{
    h->row_par ^= 1;
    for (auto& s : h->slabs) { s.v.rowsum = s.rowsumbuf[h->row_par]; s.v.rowcnt = s.rowcntbuf[h->row_par]; }
}

SlabView view_of(Handle* h, int s, int par = -1)
{
    if (par < 0) par = h->cur;
    SlabView v = h->slabs[s].v;
    v.T = h->slabs[s].Tbuf[par]; v.vval = h->slabs[s].vvalbuf[par]; v.dep_val = h->slabs[s].depbuf[par];
    return v;
}

// ---- launch shapes: the single-lattice path and the replica ensembles (R lattices per launch) take them from here ----
// Rows of Pk <= 256 columns are half-wave rows (hw); longer ones are swept in one chunk or, past 512 columns, in two
// (ch2).  npf: 16-B chunks of a class slab per thread of the streaming sweep (L > 512: pitchC >= 544, so npf >= 2).
struct RowShape { bool hw, ch2; int npf; };
RowShape row_shape(const Handle* h) { return {h->Pk <= 256, h->Pk > 512, ((SWEEP_TJ + 4) * h->pitchC / 16 + 255) / 256}; }
// (HW, CH2) of the row kernels
template <class F> void with_rows(const RowShape& rs, F&& f) { if (rs.hw) f(Yes{}, No{}); else if (!rs.ch2) f(No{}, No{}); else f(No{}, Yes{}); }
// the five (HW, NPF, CH2) shapes of k_sweep_stream
template <bool TAB, class F> void with_stream_kernel(const RowShape& rs, F&& f)
{
    if (rs.hw) f(k_sweep_stream<TAB, true, 1, false>);
    else if (rs.npf == 1) f(k_sweep_stream<TAB, false, 1, false>);
    else if (rs.npf == 2 && !rs.ch2) f(k_sweep_stream<TAB, false, 2, false>);
    else if (rs.npf == 2) f(k_sweep_stream<TAB, false, 2, true>);
    else f(k_sweep_stream<TAB, false, 3, true>);
}
// plane-marching temperature kernels: column tiles x row tiles x groups of ni planes (of every replica)
dim3 thermal_grid(int L, int nloc, int ni, int R = 1) { return dim3((L + THERM_KT - 1) / THERM_KT, (L + THERM_TJ - 1) / THERM_TJ, (nloc + ni - 1) / ni * R); }
// k_rate_table: one thread per pair of entries, grid-stride past 8192 blocks
dim3 table_grid(const SlabView& v, int R = 1)
{
    const int64_t pairs = (int64_t)v.nloc * v.L * (v.pitchT / 2);
    return dim3((unsigned)std::min<int64_t>((pairs + 255) / 256, 8192), (unsigned)R);
}
// k_sweep_plane: the 3L row sums and row counts of its plane
uint32_t plane_shmem(int L) { return (uint32_t)(3 * L * (sizeof(double) + sizeof(int))); }
// the interface lists grow while stepping: keep the interface kernel's grid at one entry per thread
void grow_ifc_grid(Handle* h, int n_list) { h->ifc_blocks = std::max(h->ifc_blocks, std::min(8192, (n_list + 255) / 256 + 64)); }

// per-call device allocation released on every return path
template <class T>
struct DevTmp {
    T* p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp&) = delete;
    DevTmp& operator=(const DevTmp&) = delete;
    ~DevTmp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void**)&p, n * sizeof(T)); }
    operator T*() const { return p; }
};

// interface list of one slab / every slab rebuilt from the membership flags, in address order
int relist_slab(Handle* h, int sl)
{
    SlabView v = view_of(h, sl);
    HIPCHK(hipMemsetAsync(v.ifc_n, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_ifc_relist, dim3((v.nloc * h->L + RELIST_ROWS - 1) / RELIST_ROWS), dim3(256), 0, h->stream, v, (const StepState*)nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}
int relist(Handle* h)
{
    for (size_t sl = 0; sl < h->slabs.size(); ++sl) CHK(relist_slab(h, (int)sl));
    return 0;
}

// extended (owned + halo, clipped) global plane range of a slab
void ext_range(const Handle* h, const Slab& s, int* a, int* b)
{
    *a = std::max(0, s.v.gi0 - 2);
    *b = std::min(h->L, s.v.gi0 + s.v.nloc + 2);
}

// f64 field: host contiguous planes [i_begin,..) -> pitched device array, planes [a,b)
int h2d_f64(Handle* h, const Slab& s, double* dst, const double* src, int i_begin, int a, int b)
{
    const int L = h->L;
    const int li = a - (s.v.gi0 - 2);
    h->cnt.bytes_h2d += (int64_t)(b - a) * L * L * 8;
    HIPCHK(hipMemcpy2DAsync(dst + (size_t)li * L * h->pitchT, (size_t)h->pitchT * 8,
                            src + (size_t)(a - i_begin) * L * L, (size_t)L * 8, (size_t)L * 8,
                            (size_t)(b - a) * L, hipMemcpyHostToDevice, h->stream));
    return 0;
}
int d2h_f64(Handle* h, const Slab& s, const double* srcd, double* dst, int i_begin, int a, int b)
{
    const int L = h->L;
    const int li = a - (s.v.gi0 - 2);
    h->cnt.bytes_d2h += (int64_t)(b - a) * L * L * 8;
    HIPCHK(hipMemcpy2DAsync(dst + (size_t)(a - i_begin) * L * L, (size_t)L * 8,
                            srcd + (size_t)li * L * h->pitchT, (size_t)h->pitchT * 8, (size_t)L * 8,
                            (size_t)(b - a) * L, hipMemcpyDeviceToHost, h->stream));
    return 0;
}

template <class SRC>
int h2d_u8(Handle* h, const Slab& s, uint8_t* dst, const SRC* src, int i_begin, int a, int b, bool check, int with_cls = 0)
{
    const int L = h->L;
    const size_t n = (size_t)(b - a) * L * L;
    CHK(ensure_scratch(h, n * sizeof(SRC)));
    h->cnt.bytes_h2d += (int64_t)(n * sizeof(SRC));
    HIPCHK(hipMemcpyAsync(h->d_scratch, src + (size_t)(a - i_begin) * L * L, n * sizeof(SRC), hipMemcpyHostToDevice, h->stream));
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    if (check) {
        if constexpr (sizeof(SRC) == 8) {
            HIPCHK(hipMemsetAsync(h->d_flag, 0, sizeof(int), h->stream));
            hipLaunchKernelGGL(k_check_range, dim3(grid), dim3(256), 0, h->stream, (const int64_t*)h->d_scratch, (int64_t)n, 0, 4, h->d_flag);
            int bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, h->d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            if (bad) return fail("state/defects values must lie in 0..4 (constants.STATES)");
        }
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pack_u8<SRC>), dim3(grid), dim3(256), 0, h->stream, s.v, dst, (const SRC*)h->d_scratch, a, b - a, with_cls);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));   // scratch is reused by the next field
    return 0;
}
template <class DST>
int d2h_u8(Handle* h, const Slab& s, const uint8_t* srcd, DST* dst, int i_begin, int a, int b)
{
    const int L = h->L;
    const size_t n = (size_t)(b - a) * L * L;
    CHK(ensure_scratch(h, n * sizeof(DST)));
    const int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_unpack_u8<DST>), dim3(grid), dim3(256), 0, h->stream, s.v, srcd, (DST*)h->d_scratch, a, b - a);
    HIPCHK(hipGetLastError());
    h->cnt.bytes_d2h += (int64_t)(n * sizeof(DST));
    HIPCHK(hipMemcpyAsync(dst + (size_t)(a - i_begin) * L * L, h->d_scratch, n * sizeof(DST), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

template <class I>
int upload_impl(Handle* h, int i_begin, int i_end, const I* state, const double* theta, const double* phi,
                const double* T, const I* defects)
{
    HIPCHK(hipSetDevice(h->dev));
    for (auto& s : h->slabs) {
        int a, b;
        ext_range(h, s, &a, &b);
        if (a < i_begin || b > i_end) return fail("upload range does not cover the slab's planes + halo");
        if (state) {
            CHK(h2d_u8<I>(h, s, s.v.state, state, i_begin, a, b, true, 1));
            ++h->state_uploads;
            HIPCHK(hipMemcpyAsync(s.prev, s.v.state, s.nS, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(hipMemsetAsync(s.v.row_chg, 0, (size_t)(s.v.nloc + 4) * h->L, h->stream));      // prev_state == state
            HIPCHK(hipMemsetAsync(s.v.ifc_in, 0, s.nT, h->stream));
            hipLaunchKernelGGL(k_ifc_rebuild, dim3(2048), dim3(256), 0, h->stream, s.v);
            CHK(relist_slab(h, (int)(&s - h->slabs.data())));
        }
        if (defects) CHK(h2d_u8<I>(h, s, s.v.defects, defects, i_begin, a, b, true));
        if (theta) CHK(h2d_f64(h, s, s.v.theta, theta, i_begin, a, b));
        if (phi) CHK(h2d_f64(h, s, s.v.phi, phi, i_begin, a, b));
        if (T) CHK(h2d_f64(h, s, s.Tbuf[h->cur], T, i_begin, a, b));
        if (theta || phi) hipLaunchKernelGGL(k_orient, dim3(1024), dim3(256), 0, h->stream, s.v);
        if (state) {
            int n = 0;
            HIPCHK(hipMemcpyAsync(&n, s.v.ifc_n, sizeof(int), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            grow_ifc_grid(h, n);
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    invalidate(h, (T || state) ? Cause::upload_T_or_state : Cause::upload);
    return 0;
}
template <class I>
int download_impl(Handle* h, int i_begin, int i_end, I* state, double* theta, double* phi, double* T, I* defects)
{
    HIPCHK(hipSetDevice(h->dev));
    for (auto& s : h->slabs) {
        int a = std::max(s.v.gi0, i_begin), b = std::min(s.v.gi0 + s.v.nloc, i_end);
        if (a >= b) continue;
        if (state) CHK(d2h_u8<I>(h, s, s.v.state, state, i_begin, a, b));
        if (defects) CHK(d2h_u8<I>(h, s, s.v.defects, defects, i_begin, a, b));
        if (theta) CHK(d2h_f64(h, s, s.v.theta, theta, i_begin, a, b));
        if (phi) CHK(d2h_f64(h, s, s.v.phi, phi, i_begin, a, b));
        if (T) CHK(d2h_f64(h, s, s.Tbuf[h->cur], T, i_begin, a, b));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- per-step launches (all asynchronous on h->stream) -----------------------------------
int launch_interface(Handle* h, bool batch, hipStream_t st, bool long_list = false)
{
    const StepState* ss = batch ? h->d_ss : nullptr;
    for (size_t s = 0; s < h->slabs.size(); ++s)
        if (long_list)
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_interface_part<1024>), dim3(2048), dim3(256), 0, st, h->kp, view_of(h, (int)s), h->d_ktab, ss);
        else
            hipLaunchKernelGGL(k_interface, dim3(h->ifc_blocks * (256 / h->ifc_block)), dim3(h->ifc_block), 0, st, h->kp,
                           view_of(h, (int)s), h->d_ktab, ss);
    HIPCHK(hipGetLastError());
    return 0;
}

// per-voxel rate table + plane L-1 deposition rates from the current temperature field (stale after an upload of T, a
// temperature update or a parameter change); it overwrites the listed voxels' entries too, so the interface kernel
// has to follow
int launch_table(Handle* h, hipStream_t st, const StepState* ss, int par)
{
    const double K0 = host_k_eff(h->p, 0, 0);
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        SlabView v = view_of(h, (int)s, par);
        hipLaunchKernelGGL(k_rate_table, table_grid(v), dim3(256), 0, st, h->kp, v, K0, ss);
        h->cnt.alg_bytes_table += (int64_t)16 * v.nloc * v.L * v.L;     // T read, table entry written
    }
    HIPCHK(hipGetLastError());
    ++h->cnt.table_updates;
    return 0;
}
int ensure_table(Handle* h, hipStream_t st, const StepState* ss)
{
    if (h->table_fresh) return 0;
    CHK(launch_table(h, st, ss, h->cur));
    h->table_fresh = true;
    invalidate(h, Cause::table_written);
    return 0;
}

StreamArgs stream_args(Handle* h, const SlabView& v)
{
    StreamArgs sa{};
    sa.T_melt = h->kp.T_melt; sa.delta_T_c = h->kp.delta_T_c; sa.kT = h->kp.kT; sa.I0 = h->kp.I0;
    sa.rate_threshold = h->kp.rate_threshold; sa.K0 = host_k_eff(h->p, 0, 0);
    sa.L = v.L; sa.gi0 = v.gi0; sa.nloc = v.nloc; sa.RJ = v.RJ; sa.pitchC = v.pitchC; sa.pitchT = v.pitchT; sa.Pk = v.Pk;
    sa.cls = v.cls; sa.T = v.T; sa.vval = v.vval; sa.dep_val = v.dep_val; sa.rowsum = v.rowsum; sa.rowcnt = v.rowcnt;
    sa.lanesum = v.lanesum; sa.lanecnt = v.lanecnt;
    sa.group_first = 0; sa.group_count = (v.nloc + STREAM_NI - 1) / STREAM_NI;
    return sa;
}

// the rate table's inputs and the table of buffer pair `par`, for the temperature tiles that write it (k_thermal_tiles16<.., TABLE>)
TableCfg table_cfg(Handle* h, const Slab& s, int par)
{
    TableCfg tb{};
    tb.T_melt = h->kp.T_melt; tb.delta_T_c = h->kp.delta_T_c; tb.kT = h->kp.kT; tb.I0 = h->kp.I0;
    tb.rate_threshold = h->kp.rate_threshold; tb.K0 = host_k_eff(h->p, 0, 0); tb.nu_dep = h->kp.nu_dep;
    tb.vval = s.vvalbuf[par]; tb.dep_val = s.depbuf[par];
    tb.lanesum = s.v.lanesum; tb.lanecnt = s.v.lanecnt;       // (one copy: a digest of the table that is current)
    return tb;
}

// interface-kernel grid from the lists' lengths as they stand (called where the host has just synchronised anyway)
int refresh_ifc_grid(Handle* h)
{
    for (auto& sl : h->slabs) {
        int n_list = 0;
        HIPCHK(hipMemcpy(&n_list, sl.v.ifc_n, sizeof(int), hipMemcpyDeviceToHost));
        grow_ifc_grid(h, n_list);
    }
    return 0;
}

// ---- collectives: RCCL on the stream, or relayed through host callbacks (bring-up / test transport) ------
inline bool multi_rank(const Handle* h) { return h->comm != nullptr || h->hc.allgather != nullptr; }
// refused by `who` (a function, or a function and what of it) unless the handle is one slab in one process; why: " (...)" or ""
int one_slab_only(const Handle* h, const std::string& who, const char* why)
{
    if (h->slabs.size() != 1 || h->nranks != 1 || multi_rank(h)) return fail(who + " needs the whole lattice in one slab of one process" + why);
    return 0;
}
// What a thermal setting rules out elsewhere, one row per setting: Mode B stepping (fn: the driver) and, its mirror image, the
// look-ahead option (fn null).  The first setting that is on refuses.
int thermal_exclusions(const ThermalSettings& s, const char* fn)
{
    const struct { bool on; const char *what, *setter, *mode_b, *ahead; } rows[] = {
        {s.remelt_on != 0, "remelting is on", "cetkmc_set_remelt", "Mode B has no melt", "the field computed ahead knows no melt"},
        {s.substeps > 1, "thermal_substeps > 1", "cetkmc_set_thermal_substeps", "Mode B updates are not sub-stepped", "the field computed ahead is one explicit step"},
        {s.scheme == CETKMC_THERMAL_IMPLICIT, "the thermal scheme is implicit", "cetkmc_set_thermal_scheme", "Mode B updates are explicit", "the field computed ahead is one explicit step"},
    };
    for (const auto& r : rows) {
        if (!r.on) continue;
        if (fn) return fail(std::string(fn) + " is refused while " + r.what + " (" + r.setter + "): " + r.mode_b);
        return fail(std::string("cetkmc_set_option: thermal_lookahead = 1 is refused while ") + r.what + " (" + r.ahead + ")");
    }
    return 0;
}

// profile 2: one more hipEvent of the batch's collective timers, recorded on the stream now (nullptr when not timing)
int comm_stamp(Handle* h)
{
    if (!h->time_comm) return 0;
    if (h->comm_ev_used == h->comm_ev.size()) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); h->comm_ev.push_back(e); }
    HIPCHK(hipEventRecord(h->comm_ev[h->comm_ev_used++], h->stream));
    return 0;
}

// in-place all-gather of `per` bytes per rank inside the device buffer `buf` (rank r's part at buf + r*per)
int comm_allgather_raw(Handle* h, void* buf, size_t per)
{
    if (h->comm) {
        NCCLCHK(g_rccl.AllGather((const char*)buf + per * h->rank, buf, per, ncclChar, h->comm, h->stream));
        return 0;
    }
    if (!h->hc.allgather) return 0;
    h->hc_stage.resize(std::max(h->hc_stage.size(), per * h->nranks));
    char* host = h->hc_stage.data();
    HIPCHK(hipMemcpyAsync(host + per * h->rank, (const char*)buf + per * h->rank, per, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->hc.allgather(h->hc.user, host + per * h->rank, host, (int64_t)per)) return fail("host all-gather callback failed");
    HIPCHK(hipMemcpyAsync(buf, host, per * h->nranks, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
int comm_allgather(Handle* h, void* buf, size_t per)
{
    CHK(comm_stamp(h));
    CHK(comm_allgather_raw(h, buf, per));
    return comm_stamp(h);
}

// Incremental step (run_steps with incremental = 1, between temperature updates): only the rows the
// previous event made stale are re-evaluated; their planes' block sums follow.
int launch_dirty_rows(Handle* h, hipEvent_t ev_a, hipEvent_t ev_b)
{
    if (ev_a) HIPCHK(hipEventRecord(ev_a, h->stream));
    // dirty rows re-evaluated, their planes' block sums reduced by the last-arriving block of each plane (one launch;
    // the arrival counters live behind the dirty list and are zero at rest)
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        SlabView v = view_of(h, (int)s);
        const StreamArgs sa = stream_args(h, v);
        const int* dl = h->d_dirty;
        int* pc = h->d_dirty + 1 + DIRTY_MAX;
        const StepState* ss = h->d_ss;
        with_rows(row_shape(h), [&](auto hw, auto ch2) {
            with_flag(h->sweep_variant == 1 || h->sweep_variant >= 3, [&](auto tab) {
                launch(k_rows_eval<tab.value, hw.value, ch2.value>, dim3(24), dim3(256), 0, h->stream, nullptr, nullptr, sa, dl, ss, h->d_blocks, pc);
            });
        });
    }
    if (ev_b) HIPCHK(hipEventRecord(ev_b, h->stream));
    HIPCHK(hipGetLastError());
    if (multi_rank(h)) CHK(comm_allgather(h, h->d_blocks, (size_t)3 * (h->L / h->nranks) * sizeof(BlockEnt)));
    h->swept = true;
    return 0;
}

// Census-free tiles in the streaming launches (option fused_tiles >= level): one slab in one process, half-wave rows, 128 < L
// (where the lattice's class bytes and rate table sit in the Infinity Cache; L <= 256 follows from the half-wave rows)
bool table_tiles(const Handle* h, int level)
{
    return h->fused_tiles >= level && h->slabs.size() == 1 && !multi_rank(h) && h->L > 128 && row_shape(h).hw;
}
size_t apply_shmem() { return APPLY_SHMEM; }
// Lane sums (option lane_sums): where the skipping census-free tiles run the deferred launches.  The look-ahead's k_thermal_fix
// writes table entries beside the loop without going through ifc_store(): with thermal_lookahead on there are no lane sums.
bool lane_table_on(const Handle* h)
{
    return h->lane_sums && h->table_lane_skip && !h->thermal_ahead && h->sweep_variant == 1 && table_tiles(h, 1) && h->slabs[0].v.lanecnt;
}
// the deferred launches read lane sums only while the table is fresh
bool lane_table_use(const Handle* h) { return lane_table_on(h) && h->lanes_fresh; }

// One full-lattice rate sweep: (rate table, if T changed) -> (interface kernel, if the listed voxels' sums are stale)
// -> sweep kernel -> block sums (+ all-gather across ranks).  ev_pre | table + interface | ev_a | sweep | ev_b |
// reduce | ev_post are the phase boundaries of cetkmc_get_counters.
int launch_sweep(Handle* h, bool batch, hipEvent_t ev_a = nullptr, hipEvent_t ev_b = nullptr, bool long_list = false,
                 hipEvent_t ev_pre = nullptr, hipEvent_t ev_post = nullptr)
{
    ++h->cnt.sweeps;
    // streaming kernels: class u8 + one f64 (rate table / T) per voxel; simple kernel: state tile + T
    for (auto& sl : h->slabs) h->cnt.alg_bytes_sweep += (int64_t)9 * sl.v.nloc * h->L * h->L;
    if (ev_pre) HIPCHK(hipEventRecord(ev_pre, h->stream));
    const int TR = SWEEP_TJ + 4;
    const size_t shmem0 = (size_t)((5 * TR * h->pitchS + 15) & ~15) + 225 * sizeof(double);
    const StepState* ss = batch ? h->d_ss : nullptr;
    const int njt = (h->L + SWEEP_TJ - 1) / SWEEP_TJ;
    if (h->sweep_variant >= 1) {
        // a pending event is applied inside the sweep launch: nothing may read the lattice before it
        if (h->pend_live && (!h->table_fresh || !h->ifc_fresh)) return fail("internal: rate table / interface sums stale under a pending event");
        CHK(ensure_table(h, h->stream, ss));
        if (!h->ifc_fresh || h->ifc_every_step) {
            CHK(launch_interface(h, batch, h->stream, long_list));
            ++h->cnt.interface_launches;
            h->ifc_fresh = true;
        }
    }
    // sweep timing of a batch (profile 1 / 3: ev_a, ev_b without the phase events): the two hipEvents ride on the launch itself
    // (launch()).  Several slabs in one process / the phase table: plain records.
    const bool ext = ev_a && ev_b && !ev_pre && h->slabs.size() == 1 && h->sweep_variant >= 1;
    const hipEvent_t xa = ext ? ev_a : nullptr, xb = ext ? ev_b : nullptr;
    if (ev_a && !ext) HIPCHK(hipEventRecord(ev_a, h->stream));
    const int sv = (h->sweep_auto && h->sweep_variant == 1 && h->L <= 128) ? 4 : h->sweep_variant;      // effective sweep kernel
    const RowShape rs = row_shape(h);
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        SlabView v = view_of(h, (int)s);
        const StreamArgs sa = stream_args(h, v);
        if (sv == 4) {
            // census-free table sweep, one 16-wave block per owned plane, block sums folded in the same launch
            with_rows(rs, [&](auto hw, auto ch2) {
                launch(k_sweep_plane<hw.value, ch2.value>, dim3((unsigned)v.nloc), dim3(1024), plane_shmem(h->L), h->stream, xa, xb, sa, ss, h->d_blocks);
            });
        } else if (sv == 3) {
            // census-free table sweep: class bytes + rate table streamed once, no LDS
            const int ipp = rs.hw ? (h->L + 1) / 2 : h->L;
            const int64_t n_items = (int64_t)ipp * v.nloc;
            const dim3 g((unsigned)((n_items + 4 * TABLE_IPW - 1) / (4 * TABLE_IPW)));
            with_rows(rs, [&](auto hw, auto ch2) {
                launch(k_sweep_table<hw.value, ch2.value>, g, dim3(256), 0, h->stream, xa, xb, sa, ss);
            });
        } else if (h->sweep_variant >= 1 && h->pend_live) {
            // the previous step's event is applied by one extra workgroup (blockIdx 0) of this launch (run_steps defers
            // only under the streaming sweep with the rate table, and only where rows are half-wave rows)
            ApplyArgs X{h->kp, (const SlabView*)dviews(h), h->d_pend, h->d_ss, h->pend_cfg, (const double*)h->d_u_defect,
                        (const double*)h->d_u_np, (const double*)h->d_ktab, h->d_log_total, h->d_log_event, h->d_log_nev};
            if (table_tiles(h, 1))      // LDS: the apply block's KParams + SlabView + PendRec copy alone; the tiles the selection
                                        // launch has not run (launch_select_pend)
                with_flag(h->table_lane_skip != 0, [&](auto ls) {
                    with_flag(lane_table_use(h), [&](auto lu) {
                        const int late = table_tile_count(h->L, v.nloc, true) - h->pend_early;
                        launch(k_sweep_stream_apply<true, 1, false, true, ls.value, ls.value && lu.value>, dim3(late + 1), dim3(256), apply_shmem(), h->stream, xa, xb, sa, h->d_ss, X, h->pend_early);
                    });
                });
            else
                launch(k_sweep_stream_apply<true, 1, false>, dim3(sa.group_count * njt + 1), dim3(256), h->shmem_stream, h->stream, xa, xb, sa, h->d_ss, X, 0);
        } else if (h->lane_sweep && lane_table_use(h)) {
            // a plain launch on a fresh lane table: the lane-sum tiles of the deferred launches over the full tile range
            // (lane_table_use(): sweep_variant 1, table_tiles(), table_lane_skip)
            launch(k_sweep_stream<true, true, 1, false, true, true, false, true>, dim3(table_tile_count(h->L, v.nloc, true)), dim3(256), 0, h->stream, xa, xb, sa, ss);
        } else if (h->sweep_variant == 1 && table_tiles(h, 2)) {
            // (a plain launch where the lane table is stale builds it: the table, the interface kernel and the lattice are current here)
            const bool build = lane_table_on(h) && !h->lanes_fresh;
            with_flag(h->table_lane_skip != 0, [&](auto ls) {
                with_flag(build, [&](auto lb) {
                    launch(k_sweep_stream<true, true, 1, false, true, ls.value, lb.value>, dim3(table_tile_count(h->L, v.nloc, true)), dim3(256), 0, h->stream, xa, xb, sa, ss);
                });
            });
            if (build) { h->lanes_fresh = true; ++h->cnt_lane_builds; }
        } else if (h->sweep_variant >= 1) {
            auto go = [&](auto k) { launch(k, dim3(sa.group_count * njt), dim3(256), h->shmem_stream, h->stream, xa, xb, sa, ss); };
            if (h->sweep_variant == 1 && lane_table_on(h) && !h->lanes_fresh) {      // the building plain launch (half-wave rows)
                go(k_sweep_stream<true, true, 1, false, false, false, true>);
                h->lanes_fresh = true; ++h->cnt_lane_builds;
            }
            else if (h->sweep_variant == 1) with_stream_kernel<true>(rs, go); else with_stream_kernel<false>(rs, go);
        } else {
            hipLaunchKernelGGL(k_sweep_simple, dim3(v.nloc * njt), dim3(256), shmem0, h->stream, h->kp, v, h->d_ktab, ss);
        }
    }
    if (ev_b && !ext) HIPCHK(hipEventRecord(ev_b, h->stream));
    if (sv != 4)          // (variant 4 folds the block sums in the sweep launch)
        for (size_t s = 0; s < h->slabs.size(); ++s) {
            SlabView v = view_of(h, (int)s);
            hipLaunchKernelGGL(k_plane_reduce, dim3(3 * v.nloc), dim3(64), 0, h->stream, v, h->d_blocks, ss);
        }
    HIPCHK(hipGetLastError());
    if (multi_rank(h)) CHK(comm_allgather(h, h->d_blocks, (size_t)3 * (h->L / h->nranks) * sizeof(BlockEnt)));
    if (ev_post) HIPCHK(hipEventRecord(ev_post, h->stream));
    h->swept = true;
    return 0;
}

int launch_select(Handle* h, const BatchCfg& cfg, double r_direct, int info_only)
{
    hipLaunchKernelGGL(k_select, dim3(1), dim3(256), 0, h->stream, h->kp, (const SlabView*)dviews(h),
                       (int)h->slabs.size(), h->L, h->PB, (const BlockEnt*)h->d_blocks, h->d_ss, cfg,
                       (const double*)h->d_u_pick, r_direct, (const double*)h->d_ktab,
                       h->d_events_all + h->my_first, info_only, h->sweep_variant >= 1 ? 1 : 0);
    HIPCHK(hipGetLastError());
    if (multi_rank(h) && !info_only) CHK(comm_allgather(h, h->d_events_all, sizeof(cetkmc_event)));
    return 0;
}

// selection + application of one batched step: one fused launch in a single process, select / all-gather / apply
// across ranks
int launch_select_apply(Handle* h, const BatchCfg& cfg, int eval_touched, int* dirty, int64_t cur_hint)
{
    if (!multi_rank(h)) {
        with_flag(h->sweep_variant >= 1, [&](auto ifc) {
            launch(k_select_apply<ifc.value>, dim3(1), dim3(256), 0, h->stream, nullptr, nullptr, h->kp, dviews(h), (int)h->slabs.size(),
                   h->L, h->PB, h->d_blocks, h->d_ss, cfg, h->d_u_pick, h->d_ktab, h->d_events_all + h->my_first, ifc.value ? 1 : 0,
                   h->d_u_defect, h->d_u_np, h->d_log_total, h->d_log_event, h->d_log_nev, eval_touched, dirty, (long long)cur_hint);
        });
        HIPCHK(hipGetLastError());
        return 0;
    }
    CHK(launch_select(h, cfg, 0.0, 0));
    hipLaunchKernelGGL(k_apply_batch, dim3(1), dim3(64), 0, h->stream, h->kp, (const SlabView*)dviews(h),
                       (int)h->slabs.size(), h->L, (const cetkmc_event*)h->d_events_all, h->G, h->d_ss, cfg,
                       (const double*)h->d_u_defect, (const double*)h->d_u_np, h->d_log_total, h->d_log_event,
                       h->d_log_nev, (const double*)h->d_ktab, eval_touched, dirty);
    HIPCHK(hipGetLastError());
    return 0;
}

// selection of a deferred step (single process): the event and its carry go to d_pend, the next sweep launch applies them.
// Option early_tiles, where that launch runs the census-free tiles: the first E tiles of its range run here, beside the
// selection block, and store into the other row-sum pair, which then becomes the current one -- the next sweep launch stores
// the remaining rows into it, and its reduce and selection read it.
int launch_select_pend(Handle* h, const BatchCfg& cfg, int64_t cur_hint)
{
    h->pend_early = 0;
    if (h->early_tiles != 0 && table_tiles(h, 1)) {
        Slab& sl = h->slabs[0];
        const int count = table_tile_count(h->L, sl.v.nloc, true);
        const int E = h->early_tiles < 0 ? count / 4 : std::min(h->early_tiles, count);
        if (h->poison_alt_rows) HIPCHK(hipMemsetAsync(sl.rowsumbuf[h->row_par ^ 1], 0xFF, sl.nR, h->stream));
        const SlabView* sel_views = dviews(h);      // the selection reads the current pair
        flip_rows(h);
        const StreamArgs sa = stream_args(h, view_of(h, 0));      // the tiles write the other one
        with_flag(h->table_lane_skip != 0, [&](auto ls) { with_flag(lane_table_use(h), [&](auto lu) {
            const int G = h->early_blocks > 0 ? std::min(h->early_blocks, E) : E;
            launch(k_select_pend_tiles<ls.value, ls.value && lu.value>, dim3(G + 1), dim3(256), 0, h->stream, nullptr, nullptr, h->kp, sel_views, (int)h->slabs.size(), h->L,
                   h->PB, (const BlockEnt*)h->d_blocks, h->d_ss, cfg, (const double*)h->d_u_pick, (const double*)h->d_ktab, h->d_pend,
                   (const double*)h->d_u_defect, (const double*)h->d_u_np, (long long)cur_hint, sa, E);
        }); });
        HIPCHK(hipGetLastError());
        h->pend_early = E;
        h->cnt.early_tiles += E;
        return 0;
    }
    hipLaunchKernelGGL(k_select_pend, dim3(1), dim3(256), 0, h->stream, h->kp, (const SlabView*)dviews(h),
                       (int)h->slabs.size(), h->L, h->PB, (const BlockEnt*)h->d_blocks, h->d_ss, cfg,
                       (const double*)h->d_u_pick, (const double*)h->d_ktab, h->d_pend, (const double*)h->d_u_defect,
                       (const double*)h->d_u_np, (long long)cur_hint);
    HIPCHK(hipGetLastError());
    return 0;
}

// neighbour exchange along the slab axis: `bytes` from send_lo to rank-1 / send_hi to rank+1 (device pointers), the
// neighbours' counterparts into recv_lo / recv_hi.  End ranks skip the missing side (its recv buffer is left alone).
int comm_exchange_raw(Handle* h, const void* send_lo, void* recv_lo, const void* send_hi, void* recv_hi, size_t bytes);
int comm_exchange(Handle* h, const void* send_lo, void* recv_lo, const void* send_hi, void* recv_hi, size_t bytes)
{
    if (h->nranks <= 1) return 0;
    CHK(comm_stamp(h));
    CHK(comm_exchange_raw(h, send_lo, recv_lo, send_hi, recv_hi, bytes));
    return comm_stamp(h);
}
int comm_exchange_raw(Handle* h, const void* send_lo, void* recv_lo, const void* send_hi, void* recv_hi, size_t bytes)
{
    if (h->nranks <= 1) return 0;
    const bool lo = h->rank > 0, hi = h->rank < h->nranks - 1;
    if (h->comm) {
        NCCLCHK(g_rccl.GroupStart());
        if (lo) {
            NCCLCHK(g_rccl.Send(send_lo, bytes, ncclChar, h->rank - 1, h->comm, h->stream));
            NCCLCHK(g_rccl.Recv(recv_lo, bytes, ncclChar, h->rank - 1, h->comm, h->stream));
        }
        if (hi) {
            NCCLCHK(g_rccl.Send(send_hi, bytes, ncclChar, h->rank + 1, h->comm, h->stream));
            NCCLCHK(g_rccl.Recv(recv_hi, bytes, ncclChar, h->rank + 1, h->comm, h->stream));
        }
        NCCLCHK(g_rccl.GroupEnd());
    } else if (h->hc.exchange) {
        h->hc_stage.resize(std::max(h->hc_stage.size(), 4 * bytes));
        char* host = h->hc_stage.data();           // [send_lo | send_hi | recv_lo | recv_hi]
        if (lo) HIPCHK(hipMemcpyAsync(host, send_lo, bytes, hipMemcpyDeviceToHost, h->stream));
        if (hi) HIPCHK(hipMemcpyAsync(host + bytes, send_hi, bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->hc.exchange(h->hc.user, lo ? h->rank - 1 : -1, hi ? h->rank + 1 : -1, host, host + 2 * bytes, host + bytes, host + 3 * bytes,
                           (int64_t)bytes))
            return fail("host neighbour-exchange callback failed");
        if (lo) HIPCHK(hipMemcpyAsync(recv_lo, host + 2 * bytes, bytes, hipMemcpyHostToDevice, h->stream));
        if (hi) HIPCHK(hipMemcpyAsync(recv_hi, host + 3 * bytes, bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return 0;
}

int exchange_T_halo(Handle* h, int buf, hipStream_t st = nullptr)
{
    if (!st) st = h->stream;
    const size_t plane = (size_t)h->L * h->pitchT;   // doubles
    for (size_t s = 0; s + 1 < h->slabs.size(); ++s) {
        Slab& a = h->slabs[s];
        Slab& b = h->slabs[s + 1];
        // a's top two owned planes -> b's lower halo; b's bottom two owned planes -> a's upper halo
        HIPCHK(hipMemcpyAsync(b.Tbuf[buf], a.Tbuf[buf] + plane * a.v.nloc, 2 * plane * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(a.Tbuf[buf] + plane * (a.v.nloc + 2), b.Tbuf[buf] + plane * 2, 2 * plane * 8, hipMemcpyDeviceToDevice, st));
    }
    if (multi_rank(h) && h->nranks > 1) {
        // my bottom / top two owned planes -> the neighbours' halos; theirs -> mine (2 L^2 doubles each way, one xGMI link per side)
        Slab& s = h->slabs[0];
        double* T = s.Tbuf[buf];
        CHK(comm_exchange(h, T + plane * 2, T, T + plane * s.v.nloc, T + plane * (s.v.nloc + 2), 2 * plane * 8));
    }
    return 0;
}

ThermalCfg thermal_cfg(Handle* h, double dt, int laser, int use_latent, int scrub)
{
    ThermalCfg C{};
    C.dt = dt; C.alpha = h->p.alpha; C.inv_dx2 = h->p.inv_dx2; C.clip_lo = h->p.T_clip_lo; C.clip_hi = h->p.T_clip_hi;
    C.T_nan = h->p.T_nan; C.rho_cp = h->p.rho_cp; C.latent_coef = h->p.latent_coef;
    C.laser = laser; C.use_latent = use_latent; C.scrub = scrub; C.ni = h->therm_ni;
    return C;
}

// one application of the explicit step: a whole update (first: counted as one), or one sub-step of it
int launch_thermal_one(Handle* h, double dt, int laser, const double* d_q, int use_latent, int scrub, bool batch, bool first = true)
{
    const ThermalCfg C = thermal_cfg(h, dt, laser, use_latent, scrub);
    if (first) ++h->cnt.thermal_updates;
    for (auto& sl : h->slabs) h->cnt.alg_bytes_thermal += (int64_t)16 * sl.v.nloc * h->L * h->L;   // T read + written
    const int nxt = h->cur ^ 1;
    size_t n_fused = 0, n_lanes = 0;
    const StepState* ssp = batch ? h->d_ss : nullptr;
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        SlabView v = view_of(h, (int)s);
        const double* Tin = h->slabs[s].Tbuf[h->cur];
        double* Tout = h->slabs[s].Tbuf[nxt];
        uint8_t* prev = h->slabs[s].prev;
        if (h->thermal_variant == 1) {
            const dim3 grid = thermal_grid(h->L, v.nloc, h->therm_ni);
            if (h->L % THERM_KT == 0 && h->L % THERM16_TJ == 0 && !h->thermal_general && h->thermal_tiles16) {   // 16-row tiles (option), covering the lattice exactly
                ThermalCfg C16 = C;
                C16.ni = h->therm_ni16;
                const dim3 g16(h->L / h->thermal_kt, h->L / THERM16_TJ, (v.nloc + C16.ni - 1) / C16.ni);
                // the default tiles also write the new field's rate table (k_rate_table's work, without reading T again)
                const bool fuse = h->thermal_table && h->thermal_rpt == 2 && h->thermal_kt == 256 && h->sweep_variant >= 1;
                if (fuse) { ++n_fused; h->cnt.alg_bytes_table += (int64_t)8 * v.nloc * v.L * v.L; }      // table entry written (T not re-read)
                // ... and the lane table of those entries (option lane_build): 8 B node + 1 B count per chunk of 8
                const bool lanes = fuse && h->lane_build && lane_table_on(h);
                if (lanes) { ++n_lanes; h->cnt.alg_bytes_table += (int64_t)9 * v.nloc * v.L * (v.pitchT / 8); }
                with_source(laser, use_latent, [&](auto la, auto lt) {
                    auto go = [&](auto k, unsigned threads, const TableCfg& tb) {
                        launch(k, g16, dim3(threads), 0, h->stream, nullptr, nullptr, v, Tin, Tout, prev, d_q, C16, ssp, tb);
                    };
                    if (lanes) go(k_thermal_tiles16<la.value, lt.value, 2, 256, true, true>, 1024, table_cfg(h, h->slabs[s], nxt));
                    else if (fuse) go(k_thermal_tiles16<la.value, lt.value, 2, 256, true>, 1024, table_cfg(h, h->slabs[s], nxt));
                    else if (h->thermal_rpt == 2 && h->thermal_kt == 128) go(k_thermal_tiles16<la.value, lt.value, 2, 128>, 512, TableCfg{});
                    else if (h->thermal_rpt == 2) go(k_thermal_tiles16<la.value, lt.value, 2, 256>, 1024, TableCfg{});
                    else go(k_thermal_tiles16<la.value, lt.value, 4, 256>, 512, TableCfg{});
                });
            } else if (h->L % THERM_KT == 0 && h->L % THERM_TJ == 0 && !h->thermal_general) {      // the 8-row tiles cover the lattice exactly
                with_source(laser, use_latent, [&](auto la, auto lt) {
                    launch(k_thermal_tiles<la.value, lt.value>, grid, dim3(256), 0, h->stream, nullptr, nullptr, v, Tin, Tout, prev, d_q, C, ssp);
                });
            } else {
                hipLaunchKernelGGL(k_thermal_march, grid, dim3(256), 0, h->stream, v, Tin, Tout, prev, d_q, C, ssp);
            }
        } else {
            hipLaunchKernelGGL(k_thermal, dim3((h->L + 255) / 256, h->L, v.nloc), dim3(256), 0, h->stream, v, Tin, Tout,
                               (const uint8_t*)prev, d_q, C, ssp);
        }
    }
    HIPCHK(hipGetLastError());
    CHK(exchange_T_halo(h, nxt));
    if (laser && use_latent) {
        for (auto& s : h->slabs) {
            if (h->thermal_variant != 1)      // the marching kernel brings prev_state level with state itself (changed rows)
                HIPCHK(hipMemcpyAsync(s.prev, s.v.state, s.nS, hipMemcpyDeviceToDevice, h->stream));
            hipLaunchKernelGGL(k_clear_row_flags, dim3(64), dim3(256), 0, h->stream, s.v, batch ? (const StepState*)h->d_ss : nullptr);
        }
        HIPCHK(hipGetLastError());
    }
    h->cur = nxt;
    const bool wrote_table = n_fused == h->slabs.size();      // every slab's update wrote its table as well
    invalidate(h, wrote_table ? Cause::thermal_update_wrote_table : Cause::thermal_update);
    if (wrote_table) { h->table_fresh = true; ++h->cnt.table_updates; }
    // ... and its lane table (lane_table_on(): one slab).  The interface kernel that has to follow poisons the chunk of every
    // entry it writes; whatever else writes entries or class bytes outside the batched apply clears the flag again (invalidate())
    if (wrote_table && n_lanes == h->slabs.size()) { h->lanes_fresh = true; ++h->cnt_lane_builds_thermal; }
    return 0;
}

// ---- sub-stepped updates (thermal_sub.hpp) ---------------------------------------------------------
// sub-steps per k_thermal_sub launch on this handle; 1: the plain path (several in-process slabs have only two halo planes)
int substep_block_of(const Handle* h)
{
    if (h->slabs.size() != 1 || multi_rank(h) || h->thermal_variant != 1) return 1;
    if (h->substep_block) return h->substep_block;
    return h->L > SUB_PLAIN_L ? SUB_SDEFAULT : 1;       // the measured default (thermal_sub.hpp)
}
// planes per block of k_thermal_sub: as few plane groups as fill the device once (every group recomputes 2 S rim planes)
int substep_planes_of(Handle* h, int S)
{
    if (h->substep_planes) return h->substep_planes;
    if (!h->n_cu && hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, h->dev) != hipSuccess) { (void)hipGetLastError(); h->n_cu = 256; }
    const int tiles = ((h->L + SUB_EK - 2 * S - 1) / (SUB_EK - 2 * S)) * ((h->L + SUB_EJ - 2 * S - 1) / (SUB_EJ - 2 * S));
    const int groups = std::max(1, h->n_cu / tiles), nloc = h->slabs[0].v.nloc;
    return std::max((nloc + groups - 1) / groups, std::min(nloc, 8));
}
template <int LASER, int S>
void launch_sub_S(Handle* h, const SlabView& v, const double* Tin, double* Tout, const double* d_q, const ThermalCfg& C, const StepState* ssp)
{
    const dim3 grid((h->L + SUB_EK - 2 * S - 1) / (SUB_EK - 2 * S), (h->L + SUB_EJ - 2 * S - 1) / (SUB_EJ - 2 * S), (v.nloc + C.ni - 1) / C.ni);
    launch(k_thermal_sub<LASER, S>, grid, dim3(SUB_THREADS), 0, h->stream, nullptr, nullptr, v, Tin, Tout, d_q, C, ssp);
}
// m further sub-steps of dt_s on a one-slab handle, S per launch (the last launch takes the remainder)
int launch_thermal_sub(Handle* h, double dt_s, int laser, const double* d_q, int m, int S, bool batch)
{
    const StepState* ssp = batch ? h->d_ss : nullptr;
    while (m > 0) {
        const int s = std::min(m, S), nxt = h->cur ^ 1;
        ThermalCfg C = thermal_cfg(h, dt_s, laser, 0, 0);
        C.ni = substep_planes_of(h, s);
        const SlabView v = view_of(h, 0);
        const double* Tin = h->slabs[0].Tbuf[h->cur];
        double* Tout = h->slabs[0].Tbuf[nxt];
        with_flag(laser != 0, [&](auto la) {
            static_assert(SUB_SMAX == 4, "one case per S");
            switch (s) {
            case 1: launch_sub_S<la.value, 1>(h, v, Tin, Tout, d_q, C, ssp); break;
            case 2: launch_sub_S<la.value, 2>(h, v, Tin, Tout, d_q, C, ssp); break;
            case 3: launch_sub_S<la.value, 3>(h, v, Tin, Tout, d_q, C, ssp); break;
            default: launch_sub_S<la.value, 4>(h, v, Tin, Tout, d_q, C, ssp); break;
            }
        });
        HIPCHK(hipGetLastError());
        h->cnt.alg_bytes_thermal += (int64_t)16 * v.nloc * h->L * h->L;     // T read + written, once per launch
        h->cur = nxt;
        ++h->ti.sub.launches; ++h->ti.sub.blocked_launches;
        m -= s;
    }
    invalidate(h, Cause::thermal_update);       // the table sub-step 1 may have written belongs to an intermediate field
    return 0;
}

// ---- implicit updates and their boundary conditions (thermal_imp.hpp, DESIGN.md sections 26 and 27) -------------------------
// the Thomas coefficients of one axis whose faces carry beta_lo, beta_hi, exactly as include/cetkmc.h states them; both 0: those
// of (I - r D) between insulated walls (L = 1: D = 0, the solve is the identity), bit for bit as cetkmc_implicit_coeffs states them
int implicit_coeffs_bc_host(const char* fn, int L, double r, double beta_lo, double beta_hi, double* inv, double* p)
{
    const std::string f(fn);
    if (!inv || !p) return fail(f + ": null argument");
    if (L < 1) return fail(f + ": L must be >= 1 (got " + std::to_string(L) + ")");
    if (!std::isfinite(r)) return fail(f + ": r is not finite");
    if (r < 0.0) return fail(f + ": r must be >= 0");
    if (!std::isfinite(beta_lo) || !std::isfinite(beta_hi)) return fail(f + ": beta is not finite");
    if (beta_lo < 0.0 || beta_hi < 0.0) return fail(f + ": beta must be >= 0");
    inv[0] = 1.0 / ((L == 1) ? 1.0 + r * (beta_lo + beta_hi) : 1.0 + r * (1.0 + beta_lo));
    p[0] = r * inv[0];
    for (int m = 1; m < L; ++m) {
        const double diag = (m < L - 1) ? (1.0 + 2.0 * r) : (1.0 + r * (1.0 + beta_hi));
        inv[m] = 1.0 / (diag - r * p[m - 1]);
        p[m] = r * inv[m];
    }
    return 0;
}
// what both boundary setters refuse of the values, before anything changes
int boundary_values_ok(const char* fn, const cetkmc_thermal_boundary& b)
{
    const std::string f(fn);
    for (int k = 0; k < 6; ++k) {
        const std::string face = " of face " + std::to_string(k);
        if (!std::isfinite(b.beta[k])) return fail(f + ": beta" + face + " is not finite");
        if (b.beta[k] < 0.0) return fail(f + ": beta" + face + " is negative");
        if (!std::isfinite(b.T_ext[k])) return fail(f + ": T_ext" + face + " is not finite");
        if (!std::isfinite(b.ramp[k])) return fail(f + ": ramp" + face + " is not finite");
    }
    return 0;
}
bool boundary_active(const cetkmc_thermal_boundary& b)
{
    for (int k = 0; k < 6; ++k) if (b.beta[k] != 0.0) return true;
    return false;
}
// the face temperature of update ordinal u: one multiply, one add
double boundary_T(const cetkmc_thermal_boundary& b, int k, int64_t u) { return b.T_ext[k] + b.ramp[k] * (double)u; }
// a stepping call's own updates (global steps g in [step0, step0 + n), g % 20 == 0, ordinal g / 20) must all have finite T_f
int boundary_steps_ok(const char* fn, const cetkmc_thermal_boundary& b, int64_t step0, int64_t n)
{
    for (int64_t g = (step0 + 19) / 20 * 20; g < step0 + n; g += 20)
        for (int k = 0; k < 6; ++k)
            if (b.beta[k] != 0.0 && !std::isfinite(boundary_T(b, k, g / 20)))
                return fail(std::string(fn) + ": the thermal boundary's temperature of face " + std::to_string(k) + " is not finite at the update of step " +
                            std::to_string(g) + " (T_ext + ramp * " + std::to_string(g / 20) + ")");
    return 0;
}
// a device table of the handle for this r (beta null: [2][L]) or for this r and a boundary's six beta ([3][2][L]): rebuilt when
// any of them changes (a handle's L never does), the upload counted where the caller says
int ensure_coeffs(Handle* h, CoefTable& t, double r, const double* beta, int64_t* uploads)
{
    const double none[6] = {};
    const size_t L = (size_t)h->L, axes = beta ? 3 : 1;
    if (!beta) beta = none;
    if (t.d && !memcmp(&t.r, &r, sizeof r) && !memcmp(t.beta, beta, sizeof t.beta)) return 0;
    std::vector<double> tab(2 * axes * L);
    for (size_t ax = 0; ax < axes; ++ax)
        CHK(implicit_coeffs_bc_host("implicit update", h->L, r, beta[2 * ax], beta[2 * ax + 1], tab.data() + 2 * ax * L, tab.data() + (2 * ax + 1) * L));
    if (!t.d && hipMalloc((void**)&t.d, tab.size() * 8) != hipSuccess) {
        (void)hipGetLastError();
        t.d = nullptr;
        return fail("implicit update: no device memory for " + std::to_string(tab.size() * 8) + " bytes");
    }
    HIPCHK(hipStreamSynchronize(h->stream));          // launches that read the previous table
    HIPCHK(hipMemcpy(t.d, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    t.r = r;
    memcpy(t.beta, beta, sizeof t.beta);
    ++*uploads;
    return 0;
}
// the by-value boundary of one implicit step at ratio r, update ordinal u: c_f = (r * beta_f) * T_f where beta_f != 0
ImpBc imp_bc(const cetkmc_thermal_boundary& b, double r, int64_t u)
{
    ImpBc B{};
    for (int k = 0; k < 6; ++k)
        if (b.beta[k] != 0.0) {
            B.c[k] = (r * b.beta[k]) * boundary_T(b, k, u);
            B.on |= 1 << k;
        }
    return B;
}
// the by-value beam of one update: row x of the table (of the handle's own set; an ensemble's launches add the replica's)
ImpBeam imp_beam(const BeamView& b, int64_t x)
{
    const int64_t L = b.L, nu = b.n_u;
    const double* d = b.d + b.base;
    ImpBeam M{};
    M.amp = d + x; M.gj = d + nu + x * L; M.gk = d + nu + nu * L + x * L; M.fi = d + nu * (1 + 2 * L);
    M.set_of = b.set_of; M.set_stride = b.set_stride; M.depth = b.depth;
    return M;
}
// the update ordinals of a stepping call (or of one direct update: step0 = 20 u, n = 1) lie inside the beam table
int beam_steps_ok(const char* fn, const BeamView& b, int64_t step0, int64_t n)
{
    const int64_t k = updates_in(step0, n);
    if (k <= 0) return 0;
    const int64_t first = (step0 > 0 ? step0 + 19 : step0) / 20, last = first + k - 1;
    if (first < b.u0 || last >= b.u0 + b.n_u)
        return fail(std::string(fn) + ": the temperature updates of the call, ordinals " + std::to_string(first) + " to " + std::to_string(last) +
                    ", leave the beam table's rows [" + std::to_string(b.u0) + ", " + std::to_string(b.u0 + b.n_u) + ")");
    return 0;
}
// a stepping call's source arguments while a beam is set: no planes, every update inside the table
int beam_args_ok(const char* fn, const BeamView& b, const double* q_planes, int64_t n_q, int64_t step0, int64_t n)
{
    if (q_planes || n_q)
        return fail(std::string(fn) + ": a beam is set, so the updates' sources are rows of its table: q_planes must be NULL and n_q 0");
    return beam_steps_ok(fn, b, step0, n);
}
// ---- one plan per update ------------------------------------------------------------------------------------------------------
// What the settings make of one temperature update of dt, update ordinal u (0 in a direct call, g / 20 at global step g of a
// stepping call: a boundary's face temperatures follow it): n steps of dt_s at ratio r, explicit or implicit, the latter between
// insulated walls or (bc) with the six addends B by value.  A handle's update and an ensemble's are launched and counted from it.
// source: a laser-mode update; with a beam set it reads row u - u0 of the table (M by value) instead of a plane.
struct UpdatePlan { int n; double dt_s, r; bool implicit, bc; ImpBc B; bool beam; int64_t row; ImpBeam M; };
UpdatePlan plan_update(const ThermalSettings& s, const cetkmc_params& p, double dt, int64_t u, bool source = false)
{
    UpdatePlan P{};
    P.n = s.substeps;
    P.dt_s = P.n > 1 ? dt / (double)P.n : dt;
    P.r = (p.alpha * P.dt_s) * p.inv_dx2;
    P.implicit = s.scheme == CETKMC_THERMAL_IMPLICIT;
    P.bc = P.implicit && s.bc_on;
    if (P.bc) P.B = imp_bc(s.bc, P.r, u);
    P.beam = P.implicit && s.beam.on && source;
    if (P.beam) {
        P.row = u - s.beam.u0;
        if (P.row >= 0 && P.row < s.beam.n_u) P.M = imp_beam(s.beam, P.row);       // (the callers refuse any other row before they launch)
    }
    return P;
}
// the update joins the running totals: the implicit records, or the sub-step record while n > 1; launches: the blocked
// sub-step path issues fewer than n and counts its own
void count_update(ThermalInfo& ti, const UpdatePlan& P, int64_t launches)
{
    if (P.implicit) {
        ++ti.imp.updates; ti.imp.steps += P.n; ti.imp.launches += launches;
        if (P.bc) { ++ti.bc.updates; ti.bc.steps += P.n; ti.bc.launches += launches; }
        if (P.beam) { ++ti.beam.updates; ti.beam.steps += P.n; ti.beam.launches += launches; }
    } else if (P.n > 1) {
        ++ti.sub.updates; ti.sub.substeps += P.n; ti.sub.launches += launches;
    }
}
// the table an implicit plan's launches read, on handle h (an ensemble's: replica 0, for every replica), uploads counted in ti
int plan_coeffs(Handle* h, const ThermalSettings& s, const UpdatePlan& P, ThermalInfo& ti, const double** coef)
{
    CoefTable& t = P.bc ? h->coef_bc : h->coef;
    CHK(ensure_coeffs(h, t, P.r, P.bc ? s.bc.beta : nullptr, P.bc ? &ti.bc.coeff_uploads : &ti.imp.coeff_uploads));
    *coef = t.d;
    return 0;
}
ImpCfg imp_cfg(const cetkmc_params& p, const UpdatePlan& P, const double* coef, int laser, int use_latent, int scrub)
{
    ImpCfg C{};
    C.r = P.r; C.dt = P.dt_s; C.dF = 1.0 / (P.dt_s > 1e-12 ? P.dt_s : 1e-12);
    C.clip_lo = p.T_clip_lo; C.clip_hi = p.T_clip_hi; C.T_nan = p.T_nan; C.rho_cp = p.rho_cp; C.latent_coef = p.latent_coef;
    C.coef = coef; C.laser = laser; C.use_latent = use_latent; C.scrub = scrub;
    return C;
}
dim3 imp_rows_grid(int L, int nloc, int R = 1) { return dim3((unsigned)(((int64_t)nloc * L + IMP_R - 1) / IMP_R), (unsigned)R); }
dim3 imp_lines_grid(int L, int R = 1) { return dim3((unsigned)((L + 63) / 64), (unsigned)L, (unsigned)R); }
// One implicit step, three launches: of a one-slab handle (its view and pointers, R = 1, no tail) or of every replica of an
// ensemble (SlabView{}, null pointers, the replica selection as the tail).  between(): what the caller queues between the row
// pass and the line passes; the tail is taken by reference, so the line passes see a flip made there.
template <class Between, class... E>
void launch_imp_step(hipStream_t st, int L, int R, const UpdatePlan& P, const ImpCfg& C, const SlabView& v, const double* Tin, double* Tout,
                     uint8_t* prev, const double* d_q, const StepState* ssp, Between&& between, E&... e)
{
    with_boundary(P.bc, P.B, [&](auto... b) {
        with_beam(P.beam, P.M, [&](auto... m) {         // the beam rides behind the boundary, in the row pass alone
            launch(k_imp_rows<decltype(b)..., decltype(m)..., E...>, imp_rows_grid(L, L, R), dim3(IMP_R), 0, st, nullptr, nullptr, v, Tin, Tout, prev, d_q, C, ssp, b..., m..., e...);
        });
        between();
        launch(k_imp_lines<1, decltype(b)..., E...>, imp_lines_grid(L, R), dim3(64), 0, st, nullptr, nullptr, v, Tout, C, ssp, b..., e...);
        launch(k_imp_lines<0, decltype(b)..., E...>, imp_lines_grid(L, R), dim3(64), 0, st, nullptr, nullptr, v, Tout, C, ssp, b..., e...);
    });
}
// a temperature update of a one-slab handle in P.n implicit steps: three launches each, one flip each
int launch_thermal_imp(Handle* h, const UpdatePlan& P, int laser, const double* d_q, int use_latent, int scrub, bool batch)
{
    const int L = h->L;
    const double* coef = nullptr;
    if (P.beam && (P.row < 0 || P.row >= h->ts.beam.n_u)) return fail("implicit update: update ordinal outside the beam table");
    if (P.beam) d_q = nullptr;
    CHK(plan_coeffs(h, h->ts, P, h->ti, &coef));
    const StepState* ssp = batch ? h->d_ss : nullptr;
    ++h->cnt.thermal_updates;
    for (int q = 0; q < P.n; ++q) {
        const bool first = q == 0;
        const ImpCfg C = imp_cfg(h->p, P, coef, laser, first ? use_latent : 0, first ? scrub : 0);
        const int nxt = h->cur ^ 1;
        const SlabView v = view_of(h, 0);
        launch_imp_step(h->stream, L, 1, P, C, v, h->slabs[0].Tbuf[h->cur], h->slabs[0].Tbuf[nxt], h->slabs[0].prev, d_q, ssp, [] {});
        if (first && laser && use_latent)       // k_imp_rows has brought prev_state level with state on the flagged rows
            hipLaunchKernelGGL(k_clear_row_flags, dim3(64), dim3(256), 0, h->stream, v, ssp);
        HIPCHK(hipGetLastError());
        h->cnt.alg_bytes_thermal += (int64_t)96 * v.nloc * L * L;      // three passes, each: read, y written, y read, x written
        h->cur = nxt;
    }
    count_update(h->ti, P, 3 * (int64_t)P.n);
    invalidate(h, Cause::thermal_update);
    return 0;
}

// a temperature update of the handle, update ordinal u: P.n applications of the explicit step with dt / n, or as many implicit steps
int launch_thermal(Handle* h, double dt, int laser, const double* d_q, int use_latent, int scrub, bool batch, int64_t u = 0)
{
    const UpdatePlan P = plan_update(h->ts, h->p, dt, u, laser != 0);
    if (P.implicit) return launch_thermal_imp(h, P, laser, d_q, use_latent, scrub, batch);
    CHK(launch_thermal_one(h, P.dt_s, laser, d_q, use_latent, scrub, batch));
    if (P.n == 1) return 0;
    const int S = substep_block_of(h);
    count_update(h->ti, P, S > 1 ? 1 : P.n);
    if (S > 1) return launch_thermal_sub(h, P.dt_s, laser, d_q, P.n - 1, S, batch);
    for (int q = 1; q < P.n; ++q) CHK(launch_thermal_one(h, P.dt_s, laser, d_q, 0, 0, batch, false));
    return 0;
}

// Look-ahead: the temperature update that global step g will perform, and the rate table of its result, computed NOW on
// stream2 from the current field into the other buffer pair -- without the latent-heat term (k_thermal_fix adds it at
// the update, for the few voxels it concerns).  The current field does not change until then, so this is the update's
// own arithmetic, merely scheduled into the idle time of the 19 steps in between (the one-block selection kernels
// leave the chip almost empty).  Single process only (the T halo of a multi-rank run travels on the main stream).
int launch_thermal_ahead(Handle* h, int64_t g, double dt, int laser, const double* d_q, int use_latent, int scrub)
{
    h->spec.valid = false;
    if (!h->thermal_ahead || h->thermal_variant != 1 || (multi_rank(h) && h->nranks > 1)) return 0;
    const ThermalCfg C = thermal_cfg(h, dt, laser, 0, scrub);
    const int nxt = h->cur ^ 1;
    HIPCHK(hipEventRecord(h->ev_main, h->stream));
    HIPCHK(hipStreamWaitEvent(h->stream2, h->ev_main, 0));
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        SlabView v = view_of(h, (int)s);
        hipLaunchKernelGGL(k_thermal_march, thermal_grid(h->L, v.nloc, h->therm_ni), dim3(256), 0, h->stream2, v, (const double*)h->slabs[s].Tbuf[h->cur],
                           h->slabs[s].Tbuf[nxt], h->slabs[s].prev, d_q, C, (const StepState*)h->d_ss);
    }
    HIPCHK(hipGetLastError());
    CHK(exchange_T_halo(h, nxt, h->stream2));
    CHK(launch_table(h, h->stream2, (const StepState*)h->d_ss, nxt));
    HIPCHK(hipEventRecord(h->ev_spec, h->stream2));
    h->spec.valid = true; h->spec.g = g; h->spec.laser = laser; h->spec.use_latent = use_latent; h->spec.scrub = scrub;
    h->spec.dt = dt; h->spec.d_q = d_q;
    return 0;
}

// the temperature update of global step g inside a batch: the look-ahead result if it stands for exactly this update
// (then only k_thermal_fix runs on the main stream), else the synchronous kernels
int thermal_step(Handle* h, int64_t g, double dt, int laser, const double* d_q, int use_latent, int scrub)
{
    Handle::Spec& sp = h->spec;
    if (!(sp.valid && sp.g == g && sp.laser == laser && sp.use_latent == use_latent && sp.scrub == scrub && sp.dt == dt && sp.d_q == d_q)) {
        if (sp.valid) { HIPCHK(hipStreamSynchronize(h->stream2)); sp.valid = false; }     // a stale look-ahead still owns the other buffers
        return launch_thermal(h, dt, laser, d_q, use_latent, scrub, true, g / 20);       // a thermal boundary's face temperatures follow the global step (section 27)
    }
    sp.valid = false;
    const ThermalCfg C = thermal_cfg(h, dt, laser, use_latent, scrub);
    const int nxt = h->cur ^ 1;
    const double K0 = host_k_eff(h->p, 0, 0);
    ++h->cnt.thermal_updates;
    HIPCHK(hipStreamWaitEvent(h->stream, h->ev_spec, 0));
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        Slab& sl = h->slabs[s];
        SlabView v = view_of(h, (int)s);
        h->cnt.alg_bytes_thermal += (int64_t)16 * v.nloc * h->L * h->L;
        hipLaunchKernelGGL(k_thermal_fix, dim3(1024), dim3(256), 0, h->stream, h->kp, v, (const double*)sl.Tbuf[h->cur], sl.Tbuf[nxt],
                           sl.prev, d_q, C, (const StepState*)h->d_ss, (const double*)sl.vvalbuf[h->cur], sl.vvalbuf[nxt],
                           (const double*)sl.depbuf[h->cur], sl.depbuf[nxt], K0);
        if (laser && use_latent)
            hipLaunchKernelGGL(k_clear_row_flags, dim3(64), dim3(256), 0, h->stream, v, (const StepState*)h->d_ss);
    }
    HIPCHK(hipGetLastError());
    if (h->slabs.size() > 1) CHK(exchange_T_halo(h, nxt));      // the recomputed voxels may sit in a neighbour slab's halo
    h->cur = nxt;
    invalidate(h, Cause::lookahead_adopted);
    h->table_fresh = true;       // computed ahead with the field
    return 0;
}

// ---- remelting (melt.hpp) ------------------------------------------------------------------------
// what every remelt entry point refuses of a handle, before anything is allocated or launched
int melt_refusals(const Handle* h, const char* fn, double threshold)
{
    if (std::isnan(threshold)) return fail(std::string(fn) + ": the threshold is NaN");
    return one_slab_only(h, fn, " (a melt in a halo plane would need the neighbour's field)");
}
// row flags and counters of this lattice, zero, on first use
int melt_ensure(Handle* h)
{
    if (h->d_melt_block) return 0;
    const size_t nflag = ((size_t)(h->slabs[0].v.nloc + 4) * h->L + 255) / 256 * 256, bytes = nflag + MELT_NC * 8;
    if (hipMalloc(&h->d_melt_block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        h->d_melt_block = nullptr;
        return fail("remelting: no device memory for " + std::to_string(bytes) + " bytes");
    }
    HIPCHK(hipMemsetAsync(h->d_melt_block, 0, bytes, h->stream));
    h->melt.flags = (uint8_t*)h->d_melt_block;
    h->melt.cnt = (unsigned long long*)((char*)h->d_melt_block + nflag);
    return 0;
}
dim3 melt_scan_grid(const SlabView& v, int R = 1) { return dim3((unsigned)(((int64_t)v.nloc * v.L * (v.pitchT / 4) + MELT_QPB - 1) / MELT_QPB), (unsigned)R); }
dim3 melt_touch_grid(const SlabView& v, int R = 1) { return dim3((unsigned)(((int64_t)v.nloc * v.L * ((v.L + 63) / 64) + 3) / 4), (unsigned)R); }
dim3 melt_close_grid(const SlabView& v, int R = 1) { return dim3((unsigned)std::min<int64_t>(((int64_t)(v.nloc + 4) * v.L + 255) / 256, 64), (unsigned)R); }
// One melt pass, three launches with grids of shape's size: over a one-slab handle's lattice (its view, prev_state and MeltState,
// R = 1, no tail) or over every replica of an ensemble (SlabView{}, null, MeltState{}, the replicas' table, the selection as tail)
template <class... E>
void launch_melt_pass(hipStream_t st, const SlabView& shape, int R, const SlabView& v, uint8_t* prev, const MeltState& M, const MeltState* tab,
                      double threshold, const StepState* ss, const E&... e)
{
    launch(k_melt_scan<E...>, melt_scan_grid(shape, R), dim3(256), 0, st, nullptr, nullptr, v, prev, M, tab, threshold, ss, e...);
    launch(k_melt_touch<E...>, melt_touch_grid(shape, R), dim3(256), 0, st, nullptr, nullptr, v, M, tab, ss, e...);
    launch(k_melt_close<E...>, melt_close_grid(shape, R), dim3(256), 0, st, nullptr, nullptr, v, M, tab, ss, e...);
}
// one pass over the lattice of a single-slab handle, on its stream; batch: a pass-through behind an early stop
int launch_melt(Handle* h, double threshold, bool batch)
{
    const SlabView v = view_of(h, 0);
    launch_melt_pass(h->stream, v, 1, v, h->slabs[0].prev, h->melt, nullptr, threshold, batch ? h->d_ss : nullptr);
    HIPCHK(hipGetLastError());
    return 0;
}
void melt_info_from(Handle* h, const unsigned long long* c)
{
    h->melt_info.passes = (int64_t)c[MELT_PASSES]; h->melt_info.n_melted = (int64_t)c[MELT_TOTAL];
    h->melt_info.n_melted_last = (int64_t)c[MELT_LAST]; h->melt_info.n_appended = (int64_t)c[MELT_APPENDED];
}

// the update of global step g in a batch that ends before global step `end`; thermal_mode 2: from source plane *q_idx of h->d_q
int batch_thermal(Handle* h, int64_t g, int64_t end, int thermal_mode, double dt, int use_latent, int64_t* q_idx)
{
    const size_t L2 = (size_t)h->L * h->L;
    const int laser = thermal_mode == 2 ? 1 : 0, latent = laser ? use_latent : 0;
    const bool planes = laser && !h->ts.beam.on;        // a beam: the update's source is the table row of g / 20
    CHK(thermal_step(h, g, dt, laser, planes ? h->d_q + (size_t)*q_idx * L2 : nullptr, latent, 1));
    *q_idx += laser;
    if (g + 20 < end)      // the next update lies inside this batch (its source plane is on the device): look ahead
        CHK(launch_thermal_ahead(h, g + 20, dt, laser, planes ? h->d_q + (size_t)*q_idx * L2 : nullptr, latent, 1));
    return 0;
}

template <class T>
int grow(T** p, size_t* cap, size_t need)
{
    if (need <= *cap && *p) return 0;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr;
    size_t n = std::max<size_t>(need, 16);
    HIPCHK(hipMalloc((void**)p, n * sizeof(T)));
    *cap = n;
    return 0;
}

int grow_pinned(char** p, size_t* cap, size_t need)
{
    if (*cap >= need) return 0;
    if (*p) { HIPCHK(hipHostFree(*p)); *p = nullptr; *cap = 0; }
    const size_t c = std::max<size_t>(need + need / 2, 1 << 16);
    HIPCHK(hipHostMalloc((void**)p, c, hipHostMallocDefault));
    *cap = c;
    return 0;
}
// the five per-step device buffers of a batch (pick / defect uniforms, the three per-step logs) for n steps
int reserve_steps(Handle* h, size_t n)
{
    size_t c1 = h->cap_steps, c2 = h->cap_steps, c3 = h->cap_steps, c4 = h->cap_steps, c5 = h->cap_steps;
    CHK(grow(&h->d_u_pick, &c1, n));
    CHK(grow(&h->d_u_defect, &c2, n));
    CHK(grow(&h->d_log_total, &c3, n));
    CHK(grow(&h->d_log_event, &c4, n));
    CHK(grow(&h->d_log_nev, &c5, n));
    h->cap_steps = std::min({c1, c2, c3, c4, c5});
    return 0;
}
// the handle's pool of timing events / the milliseconds between two of them, added to *acc
int reserve_events(Handle* h, int64_t need)
{
    while ((int64_t)h->prof.size() < need) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); h->prof.push_back(e); }
    return 0;
}
int add_elapsed(hipEvent_t ea, hipEvent_t eb, double* acc)
{
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, ea, eb));
    *acc += t;
    return 0;
}
constexpr size_t PIN_SMALL_MAX = 1 << 20;      // larger arrays (long u_np streams, many source planes) are copied directly

void destroy_impl(Handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->dev);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->stream2) (void)hipStreamSynchronize(h->stream2);
    if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
    for (auto& s : h->slabs) {
        (void)hipFree(s.v.state); (void)hipFree(s.v.defects); (void)hipFree(s.prev); (void)hipFree(s.v.row_chg); (void)hipFree(s.v.cls);
        (void)hipFree(s.Tbuf[0]); (void)hipFree(s.Tbuf[1]); (void)hipFree(s.v.theta); (void)hipFree(s.v.phi); (void)hipFree(s.v.ovec);
        (void)hipFree(s.rowsumbuf[0]); (void)hipFree(s.rowsumbuf[1]);
        (void)hipFree(s.v.lanesum); (void)hipFree(s.v.lanecnt); (void)hipFree(s.vvalbuf[0]); (void)hipFree(s.vvalbuf[1]); (void)hipFree(s.depbuf[0]); (void)hipFree(s.depbuf[1]); (void)hipFree(s.v.ifc_in); (void)hipFree(s.v.ifc_code); (void)hipFree(s.v.ifc_list); (void)hipFree(s.v.ifc_n);
    }
    if (h->d_solid_block) (void)hipFree(h->d_solid_block);
    if (h->d_origin_block) (void)hipFree(h->d_origin_block);
    if (h->d_melt_block) (void)hipFree(h->d_melt_block);
    void* ccp[] = {h->d_cc_parent, h->d_cc_roots, h->d_cc_cid, h->d_cc_labels, h->d_cc_stats, h->d_cc_n};
    for (void* p : ccp) if (p) (void)hipFree(p);
    void* ptrs[] = {h->d_views[0], h->d_views[1], h->d_views[2], h->d_views[3], h->d_blocks, h->d_events_all, h->d_ss, h->d_dirty, h->d_pend, h->d_ktab, h->d_kp, h->d_scratch,
                    h->d_flag, h->d_qtop, h->d_u_pick, h->d_u_defect, h->d_u_np, h->d_q, h->d_log_total,
                    h->d_log_event, h->d_log_nev, h->d_sup_dom, h->d_sup_picks, h->d_sup_cnt, h->d_sup_log, h->d_sup_rmax,
                    h->d_loc_horizon, h->d_loc_capped, h->d_front_part, h->d_front_out, h->d_layer_part, h->d_layer_out, h->d_layer_eq,
                    h->coef.d, h->coef_bc.d, h->d_beam};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (h->pin_in) (void)hipHostFree(h->pin_in);
    if (h->pin_out) (void)hipHostFree(h->pin_out);
    for (auto e : h->prof) (void)hipEventDestroy(e);
    for (auto e : h->comm_ev) (void)hipEventDestroy(e);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->ev_main) (void)hipEventDestroy(h->ev_main);
    if (h->ev_spec) (void)hipEventDestroy(h->ev_spec);
    if (h->stream2 && h->own_streams) (void)hipStreamDestroy(h->stream2);
    if (h->stream && h->own_streams) (void)hipStreamDestroy(h->stream);
    delete h;
}

// ---- replica ensembles (ensemble.hpp) ------------------------------------------------------------
struct Ens {
    int L = 0, R = 0;
    std::vector<Handle*> reps;           // reps[0] is the ensemble's handle; all share its streams
    std::vector<uint8_t> frozen;         // terminated in an earlier call (until a new lattice is uploaded into the replica)
    std::vector<int64_t> uploads_seen;   // Handle::state_uploads when the replica was last stepped
    std::vector<EnsRep> table;
    EnsRep* d_table = nullptr;
    double *d_u_pick = nullptr, *d_u_defect = nullptr, *d_u_np = nullptr, *d_log_total = nullptr;
    cetkmc_event* d_log_event = nullptr;
    int64_t* d_log_nev = nullptr;
    size_t cap_pick = 0, cap_defect = 0, cap_np = 0, cap_total = 0, cap_event = 0, cap_nev = 0;
    double* d_q = nullptr;               // thermal_mode 2: [n_sets][updates of the call][L*L] source planes of the call
    size_t cap_q = 0;
    StepState* d_ss_out = nullptr;
    int* d_n_out = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // batched analysis (cetkmc_ensemble_analyze): [R][L^3] label arrays, results kept until the next call
    int *d_cc_parent = nullptr, *d_cc_cid = nullptr, *d_cc_roots = nullptr, *d_cc_labels = nullptr, *d_cc_n = nullptr, *d_cc_stats = nullptr;
    size_t cap_cc_stats = 0;
    long long *d_cc_offs = nullptr, *d_sc_offs = nullptr, *d_sc_idx = nullptr, *d_g_idx = nullptr;
    size_t cap_sc_idx = 0;
    double* d_g_T = nullptr;
    unsigned long long *d_counts = nullptr, *d_g_n = nullptr;
    std::vector<int64_t> an_clusters, an_gathered;     // per replica, of the last analysis (-1: none yet)
    int an_species = -1;
    void* d_solid_block = nullptr;       // cetkmc_ensemble_solid_begin: every replica's map, the counters [R][3], the map table [R]
    SolidMap* d_solid_maps = nullptr;    // (inside the block)
    void* d_origin_block = nullptr;      // cetkmc_ensemble_origin_begin: every replica's words and census, the map table [R], the run table [R]
    OriginMap* d_origin_maps = nullptr;  // (inside the block)
    OriginRun* d_origin_runs = nullptr;
    std::vector<OriginRun> origin_runs;  // host copy of the run table of the last stepping call
    MeltState* d_melt_tab = nullptr;     // cetkmc_ensemble_set_remelt: every replica's row flags and counters [R] (each replica owns its own)
    unsigned long long* d_melt_out = nullptr;      // [R][4] counters gathered at the end of a call
    ThermalSettings ts{};                // cetkmc_ensemble_set_remelt / _thermal_substeps / _thermal_scheme / _thermal_boundary: one for all replicas
    ThermalInfo ti{};                    // of the updates cetkmc_run_ensemble made
    double* d_beam = nullptr;            // cetkmc_ensemble_set_beam: every set of the table ts.beam names, and the replicas' sets [R]
    int32_t* d_beam_set_of = nullptr;
    std::vector<int32_t> beam_set_of;
};
// the ensemble's settings reach every replica: a direct update on a replica handle follows the ensemble (a beam: from the replica's set)
void share_thermal(Ens* e)
{
    for (size_t r = 0; r < e->reps.size(); ++r) {
        ThermalSettings& s = e->reps[r]->ts;
        s = e->ts;
        if (s.beam.on) { s.beam.base = (int64_t)e->beam_set_of[r] * s.beam.set_stride; s.beam.set_of = nullptr; }
    }
}
// every field of cetkmc_params but impurity_c / nu_dep is shared by the replicas (kernels.hpp)
bool shared_params_equal(cetkmc_params a, cetkmc_params b)
{
    a.impurity_c = b.impurity_c = 0.0; a.nu_dep = b.nu_dep = 0.0;
    return !memcmp(&a, &b, sizeof a);
}
const char* const SHARED_PARAMS_MSG = "ensemble replicas may differ in impurity_c and nu_dep only (cetkmc_params)";
std::mutex g_ens_mu;
std::map<const void*, Ens*> g_ens;        // ensemble handle (= replica 0's handle) -> ensemble

Ens* ens_of(const void* handle)
{
    std::lock_guard<std::mutex> lk(g_ens_mu);
    auto it = g_ens.find(handle);
    return it == g_ens.end() ? nullptr : it->second;
}

void destroy_ens(Ens* e)
{
    if (!e->reps.empty()) {
        (void)hipSetDevice(e->reps[0]->dev);
        (void)hipStreamSynchronize(e->reps[0]->stream);
    }
    void* ptrs[] = {e->d_table, e->d_u_pick, e->d_u_defect, e->d_u_np, e->d_log_total, e->d_log_event, e->d_log_nev, e->d_q,
                    e->d_ss_out, e->d_n_out, e->d_cc_parent, e->d_cc_cid, e->d_cc_roots, e->d_cc_labels, e->d_cc_n, e->d_cc_stats,
                    e->d_cc_offs, e->d_sc_offs, e->d_sc_idx, e->d_g_idx, e->d_g_T, e->d_counts, e->d_g_n, e->d_solid_block,
                    e->d_origin_block, e->d_melt_tab, e->d_melt_out, e->d_beam, e->d_beam_set_of};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    if (e->ev0) (void)hipEventDestroy(e->ev0);
    if (e->ev1) (void)hipEventDestroy(e->ev1);
    for (size_t r = e->reps.size(); r-- > 0;) destroy_impl(e->reps[r]);     // replica 0 (owner of the streams) last
    delete e;
}

// cetkmc_destroy of an ensemble handle: true if it was one (and is gone now)
bool destroy_ensemble_of(void* handle)
{
    Ens* e = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_ens_mu);
        auto it = g_ens.find(handle);
        if (it == g_ens.end()) return false;
        e = it->second;
        g_ens.erase(it);
    }
    destroy_ens(e);
    return true;
}

}  // namespace

// =========================================================================================
extern "C" {

const char* cetkmc_last_error(void) { return g_err.c_str(); }
int cetkmc_abi_version(void) { return CETKMC_ABI_VERSION; }
#ifndef CETKMC_SRC_HASH
#define CETKMC_SRC_HASH "unknown"
#endif
// the hash follows a marker so that the binding can read it from the file without loading the library
static const char g_src_hash[] = "cetkmc-source-hash=" CETKMC_SRC_HASH;
const char* cetkmc_source_hash(void) { return g_src_hash + 19; }

int cetkmc_struct_size(const char* name)
{
    if (!name) return -1;
#define SZ(n, t) if (!strcmp(name, n)) return (int)sizeof(t)
    SZ("params", cetkmc_params); SZ("event", cetkmc_event); SZ("sweep_info", cetkmc_sweep_info);
    SZ("run_args", cetkmc_run_args); SZ("run_result", cetkmc_run_result); SZ("super_args", cetkmc_super_args);
    SZ("counters", cetkmc_counters); SZ("host_comm", cetkmc_host_comm); SZ("ens_args", cetkmc_ens_args); SZ("ens_analysis", cetkmc_ens_analysis);
    SZ("front_stats", struct cetkmc_front_stats); SZ("layer_rec", struct cetkmc_layer_rec); SZ("texture_args", struct cetkmc_texture_args);
    SZ("grain_rec", struct cetkmc_grain_rec);
    SZ("solid_info", struct cetkmc_solid_info); SZ("solid_args", struct cetkmc_solid_args); SZ("solid_rec", struct cetkmc_solid_rec);
    SZ("origin_rec", struct cetkmc_origin_rec); SZ("local_args", cetkmc_local_args);
    SZ("remelt_info", struct cetkmc_remelt_info); SZ("substep_info", struct cetkmc_substep_info);
    SZ("implicit_info", struct cetkmc_implicit_info);
    SZ("thermal_boundary", struct cetkmc_thermal_boundary);
    SZ("boundary_info", struct cetkmc_boundary_info);
    SZ("beam", struct cetkmc_beam); SZ("beam_info", struct cetkmc_beam_info);
    SZ("shift", struct cetkmc_shift); SZ("shift_info", struct cetkmc_shift_info);
#undef SZ
    return -1;
}

// ---- origin map: the part the stepping calls use (origin.hpp; its entry points close the file) -------
constexpr int64_t ORIGIN_SEQ_LIMIT = (int64_t)1 << 36;
// a call that may absorb up to n ordinals: refused, before it does anything, when the map's clock could reach 2^36
static int origin_room(const Handle* h, int64_t n, const char* fn)
{
    if (h->origin_on && n > 0 && (n >= ORIGIN_SEQ_LIMIT || h->origin_seq + n >= ORIGIN_SEQ_LIMIT))
        return fail(std::string(fn) + ": the origin map's clock (seq " + std::to_string(h->origin_seq) + ") would reach 2^36");
    return 0;
}
// n records of the device log d_log, `group` of them per ordinal, into the handle's map: one launch on its stream, behind the
// stepping call's closing event
static int origin_absorb_log(Handle* h, const cetkmc_event* d_log, int64_t n, int64_t group)
{
    if (!h->origin_on || n <= 0) return 0;
    launch(k_origin_absorb<>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, nullptr, nullptr, d_log, (long long)n, (long long)group,
           (long long)h->origin_seq, h->L, h->origin, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    h->origin_seq += n / group;
    return 0;
}

// the kernels' own stale-row rule (kernels.hpp), for host-side checks of its footprint
int cetkmc_dirty_offset(int di, int dj) { return dirty_offset(di, dj) ? 1 : 0; }
static StaleEv stale_ev_host(int type, const int pos[2], const int target[2])
{
    StaleEv se;
    se.type = type; se.pi = pos[0]; se.pj = pos[1]; se.ti = target[0]; se.tj = target[1];
    return se;
}
int cetkmc_stale_row(int type, const int pos[2], const int target[2], int gi, int j)
{
    return stale_row(stale_ev_host(type, pos, target), gi, j) ? 1 : 0;
}
int cetkmc_lane_needs_values(uint64_t class8)
{
    return lane_needs_values(make_uint2((unsigned)class8, (unsigned)(class8 >> 32))) ? 1 : 0;
}
int cetkmc_lane_request(uint64_t class8, int count_byte)
{
    static_assert(LANE_REQ_NONE == CETKMC_LANE_REQ_NONE && LANE_REQ_VALUES == CETKMC_LANE_REQ_VALUES && LANE_REQ_SUM == CETKMC_LANE_REQ_SUM, "cetkmc.h");
    return lane_request(make_uint2((unsigned)class8, (unsigned)(class8 >> 32)), (unsigned)count_byte & 0xFFu);
}
// Inspection of the lane table (tests): whether the deferred launches would read it now, its owned chunks with a count and
// poisoned (one small kernel and a synchronisation: not for a loop), the building launches so far.
int cetkmc_lane_table(void* handle, cetkmc_lane_table_info* out)
{
    Handle* h = (Handle*)handle;
    if (!h || !out) return fail("null argument");
    *out = cetkmc_lane_table_info{};
    out->fresh = lane_table_use(h) ? 1 : 0;
    out->builds = h->cnt_lane_builds;
    out->builds_thermal = h->cnt_lane_builds_thermal;
    if (h->slabs.size() != 1 || !h->slabs[0].v.lanecnt) return 0;      // no lane table at this shape
    HIPCHK(hipSetDevice(h->dev));
    CHK(ensure_scratch(h, 2 * sizeof(unsigned long long)));
    unsigned long long* d = (unsigned long long*)h->d_scratch;
    unsigned long long got[2] = {0, 0};
    HIPCHK(hipMemsetAsync(d, 0, sizeof got, h->stream));
    hipLaunchKernelGGL(k_lane_census, dim3(256), dim3(256), 0, h->stream, h->slabs[0].v, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(got, d, sizeof got, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    out->chunks = (int64_t)h->slabs[0].v.nloc * h->L * (h->pitchT / 8);
    out->usable = (int64_t)got[0];
    out->poisoned = (int64_t)got[1];
    return 0;
}
// the owned chunks of the lane table as they stand (tests): n = nloc * L * (pitchT / 8) sums and count bytes, row by row
int cetkmc_lane_table_copy(void* handle, double* sums, uint8_t* counts, int64_t n)
{
    Handle* h = (Handle*)handle;
    if (!h || !sums || !counts) return fail("null argument");
    if (h->slabs.size() != 1 || !h->slabs[0].v.lanecnt) return fail("cetkmc_lane_table_copy: the shape has no lane table");
    const SlabView& v = h->slabs[0].v;
    const int64_t cpr = h->pitchT / 8, owned = (int64_t)v.nloc * h->L * cpr, first = (int64_t)2 * h->L * cpr;
    if (n != owned) return fail("cetkmc_lane_table_copy: n must be the owned chunks, " + std::to_string(owned));
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipMemcpyAsync(sums, v.lanesum + first, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(counts, v.lanecnt + first, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}
void cetkmc_lane_quad_node(const double* x8, int lane, double* sum, int* count)
{
    double x[8];
    for (int q = 0; q < 8; ++q) x[q] = x8[q];
    lane_quad_node(x, lane, *sum, *count);
}
double cetkmc_tree8(const double* x8)
{
    double x[8];
    for (int q = 0; q < 8; ++q) x[q] = x8[q];
    return tree8(x);
}
int cetkmc_table_tile_of(int L, int gi, int j)
{
    if (L <= 128 || L > 256 || gi < 0 || gi >= L || j < 0 || j >= L) return -1;
    return table_tile_of(L, true, gi, j);
}
int cetkmc_early_tile_row(int L, int early_tiles, int gi, int j)
{
    const int t = cetkmc_table_tile_of(L, gi, j);
    return t < 0 ? -1 : (t < early_tiles ? 1 : 0);
}
int cetkmc_stale_rows(int type, const int pos[2], const int target[2], int L, int rows[][2])
{
    const StaleEv se = stale_ev_host(type, pos, target);
    int n = 0;
    for (int c = 0; c < STALE_CAND; ++c) {          // the apply block: lane c tests candidate c
        int gi, j;
        if (!stale_candidate(se, L, c, gi, j)) continue;
        if (n < PATCH_MAX) { rows[n][0] = gi; rows[n][1] = j; }
        ++n;
    }
    return n;
}
// the table invalidate() clears by, by cause name
int cetkmc_invalidates(const char* cause)
{
    for (const CauseRow& row : INVALIDATES)
        if (cause && !strcmp(cause, row.name)) return (int)row.stale;
    return -1;
}

int cetkmc_device_count(int* n)
{
    if (!n) return fail("null argument");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail(std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *n = c;
    return 0;
}

int cetkmc_create(const cetkmc_params* p, int L, int n_slabs, const int* device_ids, void** handle)
{
    if (n_slabs < 1) return fail("n_slabs must be >= 1");
    int dev = device_ids ? device_ids[0] : 0;
    for (int s = 1; s < n_slabs && device_ids; ++s)
        if (device_ids[s] != dev)
            return fail("in-process slabs must share one device; multi-GPU runs use one process per GPU (cetkmc_create_rank)");
    if (n_slabs > 1 && L / n_slabs < 2) return fail("each slab needs at least 2 planes");
    std::vector<std::pair<int, int>> ranges;
    int base = L / n_slabs, rem = L % n_slabs, at = 0;
    for (int s = 0; s < n_slabs; ++s) { int n = base + (s < rem ? 1 : 0); ranges.push_back({at, n}); at += n; }
    return create_common(p, L, ranges, dev, n_slabs, 0, handle);
}

int cetkmc_get_unique_id(char out[128])
{
    CHK(load_rccl());
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    NCCLCHK(g_rccl.GetUniqueId(&id));
    memcpy(out, &id, 128);
    return 0;
}

int cetkmc_create_rank(const cetkmc_params* p, int L, int rank, int nranks, int device_id, const char unique_id[128],
                       void** handle)
{
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail("bad rank/nranks");
    if (L % nranks != 0) return fail("L must be divisible by the number of ranks");
    if (nranks > 1 && L / nranks < 2) return fail("each slab needs at least 2 planes");
    const int n = L / nranks;
    std::vector<std::pair<int, int>> ranges{{rank * n, n}};
    CHK(create_common(p, L, ranges, device_id, nranks, rank, handle));
    Handle* h = (Handle*)*handle;
    h->rank = rank; h->nranks = nranks;
    if (nranks > 1 || unique_id) {
        if (!unique_id) { destroy_impl(h); *handle = nullptr; return fail("unique_id required"); }
        if (load_rccl()) { destroy_impl(h); *handle = nullptr; return 1; }
        ncclUniqueId id;
        memcpy(&id, unique_id, 128);
        ncclResult_t r = g_rccl.CommInitRank(&h->comm, nranks, id, rank);
        if (r != ncclSuccess) {
            std::string m = std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r);
            destroy_impl(h); *handle = nullptr;
            return fail(m);
        }
    }
    return 0;
}

int cetkmc_create_rank_host(const cetkmc_params* p, int L, int rank, int nranks, int device_id, const cetkmc_host_comm* hc,
                            void** handle)
{
    if (!hc || !hc->allgather || !hc->exchange) return fail("host transport callbacks required");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail("bad rank/nranks");
    if (L % nranks != 0) return fail("L must be divisible by the number of ranks");
    if (nranks > 1 && L / nranks < 2) return fail("each slab needs at least 2 planes");
    const int n = L / nranks;
    std::vector<std::pair<int, int>> ranges{{rank * n, n}};
    CHK(create_common(p, L, ranges, device_id, nranks, rank, handle));
    Handle* h = (Handle*)*handle;
    h->rank = rank; h->nranks = nranks;
    h->hc = *hc;
    return 0;
}

int cetkmc_destroy(void* handle)
{
    if (destroy_ensemble_of(handle)) return 0;
    if (handle && ((Handle*)handle)->ens_member) return fail("a replica handle is released with its ensemble");
    destroy_impl((Handle*)handle);
    return 0;
}

int cetkmc_set_params(void* handle, const cetkmc_params* p)
{
    Handle* h = (Handle*)handle;
    if (!h || !p) return fail("null argument");
    HIPCHK(hipSetDevice(h->dev));
    h->p = *p; h->kp = make_kparams(*p);
    invalidate(h, Cause::set_params);
    return upload_ktab(h);
}

int cetkmc_set_option(void* handle, const char* key, int64_t value)
{
    Handle* h = (Handle*)handle;
    if (!h || !key) return fail("null argument");
    if (!strcmp(key, "sweep_variant")) {
        if (value < 0 || value > 4) return fail("sweep_variant must be 0 (simple), 1 (streaming + rate table, default), 2 (streaming, recompute), 3 (census-free table sweep) or 4 (census-free, one block per plane, block sums in the same launch)");
        h->sweep_variant = (int)value;
        h->sweep_auto = 0;          // an explicit choice stands at every lattice size
        invalidate(h, Cause::option_sweep_variant);
        return 0;
    }
    if (!strcmp(key, "interface_every_step")) { h->ifc_every_step = value ? 1 : 0; invalidate(h, Cause::option_interface_every_step); return 0; }
    if (!strcmp(key, "thermal_planes_per_block")) {
        if (value < 1 || value > 64) return fail("thermal_planes_per_block must be 1..64");
        h->therm_ni = (int)value;
        return 0;
    }
    if (!strcmp(key, "thermal_planes_per_block16")) {
        if (value < 1 || value > 64) return fail("thermal_planes_per_block16 must be 1..64");
        h->therm_ni16 = (int)value;
        return 0;
    }
    if (!strcmp(key, "thermal_lookahead")) {
        if (value) CHK(thermal_exclusions(h->ts, nullptr));
        h->thermal_ahead = value ? 1 : 0;
        h->lanes_fresh = false;         // (no lane sums beside the look-ahead: lane_table_on())
        return 0;
    }
    if (!strcmp(key, "substep_block")) {
        if (value < 0 || value > SUB_SMAX) return fail("substep_block must be 0 (default), 1 (plain path: one launch per sub-step) or 2.." + std::to_string(SUB_SMAX) + " sub-steps per k_thermal_sub launch");
        h->substep_block = (int)value;
        return 0;
    }
    if (!strcmp(key, "substep_planes")) {
        if (value < 0 || value > 4096) return fail("substep_planes must be 0 (default: one round of blocks) or 1..4096 planes per block of k_thermal_sub");
        h->substep_planes = (int)value;
        return 0;
    }
    if (!strcmp(key, "apply_in_sweep")) { h->apply_in_sweep = value ? 1 : 0; return 0; }
    if (!strcmp(key, "fused_tiles")) {
        if (value < 0 || value > 2) return fail("fused_tiles must be 0 (ring tiles), 1 (census-free tiles in the launch that applies a pending event, default) or 2 (in the plain streaming launch at that shape as well)");
        h->fused_tiles = (int)value;
        return 0;
    }
    if (!strcmp(key, "table_lane_skip")) { h->table_lane_skip = value ? 1 : 0; return 0; }
    if (!strcmp(key, "lane_sums")) {
        if (value < 0 || value > 1) return fail("lane_sums must be 0 (the tiles read table entries) or 1 (lane sums of pristine chunks, default)");
        h->lane_sums = (int)value;
        h->lanes_fresh = false;         // the next plain launch builds
        return 0;
    }
    // (neither touches lanes_fresh: the lane table is valid whoever built it, and the plain launch reads it or not)
    if (!strcmp(key, "lane_build")) { h->lane_build = value ? 1 : 0; return 0; }
    if (!strcmp(key, "lane_sweep")) { h->lane_sweep = value ? 1 : 0; return 0; }
    if (!strcmp(key, "early_tiles")) {
        if (value < -1 || value > INT32_MAX) return fail("early_tiles must be a tile count >= 0, or -1 (a quarter of the tiles)");
        h->early_tiles = (int)value;
        return 0;
    }
    if (!strcmp(key, "early_blocks")) {
        if (value < 0 || value > INT32_MAX) return fail("early_blocks must be a block count >= 0");
        h->early_blocks = (int)value;
        return 0;
    }
    if (!strcmp(key, "poison_alt_rows")) { h->poison_alt_rows = value ? 1 : 0; return 0; }
    if (!strcmp(key, "thermal_table")) { h->thermal_table = value ? 1 : 0; return 0; }
    if (!strcmp(key, "reserve_batch")) {
        // device buffers (uniform streams, per-step logs, one laser source plane per temperature update) and hipEvents of a
        // batch of `value` steps, allocated ahead of it: a bench keeps hipMalloc / hipEventCreate out of its timed region
        if (value < 0 || value > (1 << 22)) return fail("reserve_batch out of range");
        HIPCHK(hipSetDevice(h->dev));
        invalidate(h, Cause::option_reserve_batch);      // growing a buffer moves it: a batch staged before this call is gone
        const size_t n = (size_t)value;
        CHK(reserve_steps(h, n));
        CHK(grow(&h->d_u_np, &h->cap_np, 2 * n + 2 + (size_t)h->L * h->L));
        CHK(grow(&h->d_q, &h->cap_q, (n / 20 + 2) * (size_t)h->L * h->L));
        CHK(grow_pinned(&h->pin_in, &h->pin_in_cap, 2 * n * 8 + (2 * n + 2) * 8 + std::min<size_t>(PIN_SMALL_MAX, (n / 20 + 2) * (size_t)h->L * h->L * 8)));
        CHK(grow_pinned(&h->pin_out, &h->pin_out_cap, 64 + n * (16 + sizeof(cetkmc_event)) + h->slabs.size() * sizeof(int) + (h->ts.remelt_on ? 8 + 4 * 8 : 0)));
        // events: the per-phase mode (7 per step) is used on short batches only; the sampled modes need 2 per (8th) step
        return reserve_events(h, std::max<int64_t>(7 * std::min<int64_t>(value, 256), value <= 64 ? 2 * value : 2 * (value / 8 + 1)));
    }
    if (!strcmp(key, "thermal_variant")) {
        // 0: one thread per voxel; 1 (default): plane marching -- k_thermal_tiles16 (16 x 256 tiles, 1024 threads, 2 rows per
        // thread) where the tiles cover the lattice exactly (L a multiple of 256), else k_thermal_march; 2: k_thermal_march
        // everywhere; 3: 16-row tiles with 4 rows per thread (512 threads); 4: the 8-row k_thermal_tiles; 5: 16 x 128 tiles
        if (value < 0 || value > 5) return fail("thermal_variant must be 0 (simple), 1 (marching, default: 16-row tiles, 2 rows per thread), 2 (marching, general kernel only), 3 (16-row tiles, 4 rows per thread), 4 (8-row tiles) or 5 (16-row x 128-column tiles)");
        h->thermal_general = value == 2 ? 1 : 0;
        h->thermal_tiles16 = value == 4 ? 0 : 1;
        h->thermal_rpt = value == 3 ? 4 : 2;
        h->thermal_kt = value == 5 ? 128 : 256;
        if (value >= 2) value = 1;
        h->thermal_variant = (int)value;
        return 0;
    }
    return fail(std::string("unknown option ") + key);
}

int cetkmc_sync(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int cetkmc_owned_planes(void* handle, int* i0, int* i1)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    if (i0) *i0 = h->own_i0;
    if (i1) *i1 = h->own_i1;
    return 0;
}

int cetkmc_upload(void* handle, const int64_t* state, const double* theta, const double* phi, const double* T,
                  const int64_t* defects)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    return upload_impl<int64_t>(h, 0, h->L, state, theta, phi, T, defects);
}
int cetkmc_download(void* handle, int64_t* state, double* theta, double* phi, double* T, int64_t* defects)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    return download_impl<int64_t>(h, 0, h->L, state, theta, phi, T, defects);
}
int cetkmc_upload_planes(void* handle, int i_begin, int i_end, const uint8_t* state, const double* theta,
                         const double* phi, const double* T, const uint8_t* defects)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    if (i_begin < 0 || i_end > h->L || i_begin >= i_end) return fail("bad plane range");
    return upload_impl<uint8_t>(h, i_begin, i_end, state, theta, phi, T, defects);
}
int cetkmc_download_planes(void* handle, int i_begin, int i_end, uint8_t* state, double* theta, double* phi, double* T,
                           uint8_t* defects)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    if (i_begin < 0 || i_end > h->L || i_begin >= i_end) return fail("bad plane range");
    return download_impl<uint8_t>(h, i_begin, i_end, state, theta, phi, T, defects);
}

int cetkmc_set_defects(void* handle, const uint8_t* mask)
{
    Handle* h = (Handle*)handle;
    if (!h || !mask) return fail("null argument");
    HIPCHK(hipSetDevice(h->dev));
    for (auto& s : h->slabs) {
        int a, b;
        ext_range(h, s, &a, &b);
        CHK(h2d_u8<uint8_t>(h, s, s.v.defects, mask, 0, a, b, false));
    }
    invalidate(h, Cause::set_defects);
    return 0;
}

int cetkmc_set_prev_state(void* handle, const int64_t* prev_state)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->dev));
    invalidate(h, prev_state ? Cause::set_prev_state_array : Cause::set_prev_state_null);
    for (auto& s : h->slabs) {
        if (prev_state) {
            int a, b;
            ext_range(h, s, &a, &b);
            CHK(h2d_u8<int64_t>(h, s, s.prev, prev_state, 0, a, b, true));
            HIPCHK(hipMemsetAsync(s.v.row_chg, 1, (size_t)(s.v.nloc + 4) * h->L, h->stream));      // may differ anywhere
        } else {
            HIPCHK(hipMemcpyAsync(s.prev, s.v.state, s.nS, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(hipMemsetAsync(s.v.row_chg, 0, (size_t)(s.v.nloc + 4) * h->L, h->stream));
            // the membership flags stay: a voxel that has left the interface since its last evaluation (steps under
            // interface_every_step or sweep_variant 0 do not re-evaluate what they touch) still holds that evaluation's count
            // in its class byte and its sum in the table, and only the list's next evaluation brings both up to date
            hipLaunchKernelGGL(k_ifc_rebuild, dim3(2048), dim3(256), 0, h->stream, s.v);
            CHK(relist_slab(h, (int)(&s - h->slabs.data())));
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int cetkmc_thermal_cet(void* handle, double dt, int scrub_nan)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->dev));
    CHK(launch_thermal(h, dt, 0, nullptr, 0, scrub_nan, false));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int cetkmc_thermal_laser(void* handle, double dt, const double* q_top, int use_latent, int scrub_nan)
{
    Handle* h = (Handle*)handle;
    if (!h || !q_top) return fail("null argument");
    if (h->ts.beam.on) return fail("cetkmc_thermal_laser: a beam is set; cetkmc_thermal_beam makes an update from its table (or cetkmc_set_beam(handle, NULL) first)");
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipMemcpyAsync(h->d_qtop, q_top, (size_t)h->L * h->L * sizeof(double), hipMemcpyHostToDevice, h->stream));
    CHK(launch_thermal(h, dt, 1, h->d_qtop, use_latent, scrub_nan, false));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int cetkmc_rate_sweep(void* handle, cetkmc_sweep_info* info)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->dev));
    CHK(launch_sweep(h, false));
    BatchCfg cfg{};
    CHK(launch_select(h, cfg, 0.0, 1));
    StepState ss;
    HIPCHK(hipMemcpyAsync(&ss, h->d_ss, sizeof ss, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (info) { info->total = ss.total; info->n_events = ss.n_events; info->n_dep = ss.n_dep; }
    return 0;
}

int cetkmc_select(void* handle, double r, cetkmc_event* out)
{
    Handle* h = (Handle*)handle;
    if (!h || !out) return fail("null argument");
    if (!h->swept) return fail("cetkmc_select needs a preceding cetkmc_rate_sweep on the current lattice");
    HIPCHK(hipSetDevice(h->dev));
    BatchCfg cfg{};
    CHK(launch_select(h, cfg, r, 0));
    std::vector<cetkmc_event> all(h->G);
    HIPCHK(hipMemcpyAsync(all.data(), h->d_events_all, all.size() * sizeof(cetkmc_event), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    out->type = -1;
    for (auto& e : all) if (e.type >= 0) *out = e;
    if (out->type < 0) return fail("no valid events");
    return 0;
}

int cetkmc_apply(void* handle, const cetkmc_event* ev, double theta_new, double phi_new, int make_defect)
{
    Handle* h = (Handle*)handle;
    if (!h || !ev) return fail("null argument");
    if (ev->type < 0 || ev->type > 3) return fail("bad event type");
    for (int a = 0; a < 3; ++a) if (ev->pos[a] < 0 || ev->pos[a] >= h->L) return fail("event position out of range");
    if (ev->type == CETKMC_DIFF || ev->type == CETKMC_ATT)
        for (int a = 0; a < 3; ++a) if (ev->target[a] < 0 || ev->target[a] >= h->L) return fail("event target out of range");
    CHK(origin_room(h, 1, "cetkmc_apply"));
    HIPCHK(hipSetDevice(h->dev));
    cetkmc_event e = *ev;
    if (e.type == CETKMC_DEP || e.type == CETKMC_NUC) { e.theta = theta_new; e.phi = phi_new; }
    hipLaunchKernelGGL(k_apply_direct, dim3(1), dim3(64), 0, h->stream, h->kp, (const SlabView*)dviews(h),
                       (int)h->slabs.size(), e, make_defect, h->d_ss, (const double*)h->d_ktab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    invalidate(h, Cause::apply);
    if (h->origin_on) {      // the event joins the origin map under one ordinal
        launch(k_origin_absorb_one, dim3(1), dim3(64), 0, h->stream, nullptr, nullptr, e, (long long)h->origin_seq, h->L, h->origin);
        HIPCHK(hipGetLastError());
        ++h->origin_seq;
    }
    return 0;
}

int cetkmc_row_sums(void* handle, double* rowsum, int32_t* rowcnt)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    if (!h->swept) return fail("cetkmc_row_sums needs a preceding cetkmc_rate_sweep");
    HIPCHK(hipSetDevice(h->dev));
    const size_t L = h->L;
    for (auto& s : h->slabs) {
        const size_t off = (size_t)s.v.gi0 * 3 * L, n = (size_t)s.v.nloc * 3 * L;
        if (rowsum) HIPCHK(hipMemcpyAsync(rowsum + off, s.v.rowsum, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (rowcnt) HIPCHK(hipMemcpyAsync(rowcnt + off, s.v.rowcnt, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int cetkmc_enumerate_events(void* handle, cetkmc_event* buf, int64_t cap, int64_t* n)
{
    Handle* h = (Handle*)handle;
    if (!h || !n) return fail("null argument");
    HIPCHK(hipSetDevice(h->dev));
    CHK(launch_sweep(h, false));
    const size_t L = h->L;
    int64_t total = 0;
    std::vector<std::vector<int64_t>> offs(h->slabs.size());
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        Slab& sl = h->slabs[s];
        const size_t rows = (size_t)sl.v.nloc * 3 * L;
        std::vector<int32_t> cnt(rows);
        HIPCHK(hipMemcpyAsync(cnt.data(), sl.v.rowcnt, rows * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        offs[s].resize(rows);
        for (size_t r = 0; r < rows; ++r) { offs[s][r] = total; total += cnt[r]; }
    }
    *n = total;
    if (!buf || cap <= 0 || total == 0) return 0;
    const int64_t m = std::min<int64_t>(cap, total);
    DevTmp<cetkmc_event> d_out;
    HIPCHK(d_out.alloc((size_t)m));
    for (size_t s = 0; s < h->slabs.size(); ++s) {
        const size_t rows = offs[s].size();
        DevTmp<int64_t> d_off;
        HIPCHK(d_off.alloc(rows));
        HIPCHK(hipMemcpyAsync(d_off, offs[s].data(), rows * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_enumerate, dim3((unsigned)((rows + 63) / 64)), dim3(64), 0, h->stream, h->kp, view_of(h, (int)s),
                           (const double*)h->d_ktab, (const int64_t*)d_off.p, d_out.p, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    HIPCHK(hipMemcpy(buf, d_out, (size_t)m * sizeof(cetkmc_event), hipMemcpyDeviceToHost));
    int64_t rank = 0;
    for (int64_t e = 0; e < m; ++e) if (buf[e].type == CETKMC_DEP) buf[e].dep_rank = rank++;
    return 0;
}

// argument checks / host inputs of a batch -> the handle's device buffers (grown as needed); shared by cetkmc_stage_inputs /
// cetkmc_run_steps
static int check_run_args(const cetkmc_run_args* a, bool need_ptrs, bool beam)
{
    const int64_t n = a->n_steps;
    if (n < 0) return fail("n_steps < 0");
    if (a->rng_mode < 0 || a->rng_mode > 2) return fail("rng_mode must be 0 (reference stream), 1 (counter species draw) or 2 (all counter based)");
    const bool streams = a->rng_mode != 2;          // rng_mode 2 draws every uniform from (seed, step, key): no host streams
    if (need_ptrs && streams && n > 0 && !a->u_pick) return fail("u_pick required");
    if (need_ptrs && streams && a->defect_fraction > 0.0 && n > 0 && !a->u_defect) return fail("u_defect required when defect_fraction > 0");
    if (need_ptrs && streams && a->np_cap > 0 && !a->u_np) return fail("u_np required");
    const int64_t n_therm = a->thermal_mode ? updates_in(a->step0, n) : 0;
    if (a->thermal_mode == 2 && !beam && (n_therm > a->n_q || (need_ptrs && n_therm > 0 && !a->q_planes)))
        return fail("thermal_mode 2 needs one q plane per thermal update in the batch");
    return 0;
}

static int upload_run_inputs(Handle* h, const cetkmc_run_args* a)
{
    const int64_t n = a->n_steps, n_therm = a->thermal_mode ? updates_in(a->step0, n) : 0;
    const size_t L2 = (size_t)h->L * h->L;
    CHK(reserve_steps(h, (size_t)n));
    CHK(grow(&h->d_u_np, &h->cap_np, (size_t)std::max<int64_t>(a->np_cap, 2)));
    const bool planes = a->thermal_mode == 2 && !h->ts.beam.on;        // a beam: no plane travels
    if (planes) CHK(grow(&h->d_q, &h->cap_q, (size_t)std::max<int64_t>(n_therm, 1) * L2));
    // the small arrays travel through the page-locked staging buffer (queued copies); a large one goes directly
    struct Part { void* dst; const void* src; size_t bytes; };
    const bool streams = a->rng_mode != 2;
    const Part parts[4] = {{h->d_u_pick, a->u_pick, (streams && n > 0 && a->u_pick) ? (size_t)n * 8 : 0},
                           {h->d_u_defect, a->u_defect, (streams && n > 0 && a->u_defect) ? (size_t)n * 8 : 0},
                           {h->d_u_np, a->u_np, (streams && a->np_cap > 0 && a->u_np) ? (size_t)a->np_cap * 8 : 0},
                           {h->d_q, a->q_planes, (planes && n_therm > 0) ? (size_t)n_therm * L2 * 8 : 0}};
    size_t small = 0;
    for (const Part& q : parts) if (q.bytes && q.bytes <= PIN_SMALL_MAX) small += q.bytes;
    // the staging buffer may still feed the copies of the previous call: they are complete (every stepping call ends with a
    // stream synchronisation), so it can be rewritten
    CHK(grow_pinned(&h->pin_in, &h->pin_in_cap, small));
    size_t off = 0;
    for (const Part& q : parts) {
        if (!q.bytes) continue;
        if (q.bytes <= PIN_SMALL_MAX) {
            memcpy(h->pin_in + off, q.src, q.bytes);
            HIPCHK(hipMemcpyAsync(q.dst, h->pin_in + off, q.bytes, hipMemcpyHostToDevice, h->stream));
            off += q.bytes;
        } else {
            HIPCHK(hipMemcpyAsync(q.dst, q.src, q.bytes, hipMemcpyHostToDevice, h->stream));
        }
    }
    h->cnt.bytes_h2d += (n > 0 ? n * 8 : 0) + (n > 0 && a->u_defect ? n * 8 : 0) + std::max<int64_t>(a->np_cap, 0) * 8 +
                        (planes ? n_therm * (int64_t)L2 * 8 : 0);
    return 0;
}

int cetkmc_stage_inputs(void* handle, const cetkmc_run_args* a)
{
    Handle* h = (Handle*)handle;
    if (!h || !a) return fail("null argument");
    if (h->in_ensemble) return fail("an ensemble replica is stepped by cetkmc_run_ensemble");
    if (h->ts.beam.on && a->thermal_mode == 2) CHK(beam_args_ok("cetkmc_stage_inputs", h->ts.beam, a->q_planes, a->n_q, a->step0, a->n_steps));
    invalidate(h, Cause::batch_begin);
    CHK(check_run_args(a, true, h->ts.beam.on));
    HIPCHK(hipSetDevice(h->dev));
    CHK(upload_run_inputs(h, a));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->staged.valid = true;
    h->staged.step0 = a->step0; h->staged.n_steps = a->n_steps; h->staged.np_cap = a->np_cap; h->staged.n_q = a->n_q;
    h->staged.thermal_mode = a->thermal_mode; h->staged.has_defect = a->u_defect != nullptr;
    return 0;
}

// hipEvents of a profiled batch (cetkmc_run_args.profile; Handle::prof).  1: two events per step around the rate-sweep
// kernel (bench roofline); 3: like 1 but only every 8th step (every 4th in batches of <= 64 steps) carries the two events (a
// pair costs ~4 us of stream time); 2: seven per step (thermal | interface | sweep | reduce(+all-gather) | select+apply
// boundaries) for cetkmc_get_counters.  An event a mode does not have is nullptr.
struct ProfEvents {
    static constexpr int EPS = 7;      // events per step of profile 2
    Handle* h;
    int mode;
    int64_t n, stride;
    std::vector<char> was_thermal, was_full;      // profile 2: what each step ran
    ProfEvents(Handle* h_, int mode_, int64_t n_)
        : h(h_), mode(mode_), n(n_), stride(mode_ == 3 ? (n_ <= 64 ? 4 : 8) : 1), was_thermal(mode_ == 2 ? (size_t)n_ : 0, 0), was_full(was_thermal) {}
    int64_t needed() const { return mode == 2 ? EPS * n : mode ? 2 * ((n + stride - 1) / stride) : 0; }     // sampled steps only
    bool sampled(int64_t s) const { return mode == 1 || (mode == 3 && s % stride == 0); }
    hipEvent_t phase(int64_t s, int q) const { return mode == 2 ? h->prof[EPS * s + q] : nullptr; }
    hipEvent_t pair(int64_t s, int q) const { return sampled(s) ? h->prof[2 * (s / stride) + q] : nullptr; }
    hipEvent_t sweep(int64_t s, int q) const { return mode == 2 ? phase(s, 2 + q) : pair(s, q); }      // around the step's sweep / dirty-row kernel
    int record(int64_t s, int q) const { if (mode == 2) HIPCHK(hipEventRecord(phase(s, q), h->stream)); return 0; }
    // after the batch's synchronisation: the sweep time of the call, and (profile 2) the phase times of the counters
    int collect(cetkmc_run_result* res) const
    {
        cetkmc_counters& c = h->cnt;
        for (int64_t s = 0; s < n && mode; ++s) {
            const bool full = mode != 2 || was_full[s];
            if (full && sweep(s, 0)) { CHK(add_elapsed(sweep(s, 0), sweep(s, 1), &res->sweep_ms_total)); ++res->sweep_launches; }
            if (mode != 2) continue;
            auto ph = [&](int q, double* acc) { return add_elapsed(phase(s, q), phase(s, q + 1), acc); };
            if (full && was_thermal[s]) CHK(ph(0, &c.ms_thermal));
            if (full) CHK(ph(1, &c.ms_interface));
            CHK(ph(2, full ? &c.ms_sweep : &c.ms_dirty_rows));
            CHK(ph(3, &c.ms_reduce));
            CHK(ph(4, &c.ms_select_apply));
        }
        if (mode == 2) c.profiled_steps += n;
        return 0;
    }
};

// cetkmc_run_steps, part 1: argument checks, the staged batch (consumed or dropped), the inputs' upload
static int stage_run(Handle* h, const cetkmc_run_args* a)
{
    const int64_t n = a->n_steps;
    // all input pointers NULL: the batch's inputs were put on the device by cetkmc_stage_inputs (same batch shape)
    const bool staged = n > 0 && a->rng_mode != 2 && !a->u_pick && !a->u_defect && !a->u_np && !a->q_planes;
    CHK(check_run_args(a, !staged, h->ts.beam.on));
    const auto g = h->staged;
    invalidate(h, Cause::batch_begin);      // a staged batch is consumed (or dropped) by the next stepping call
    if (staged) {
        if (!g.valid) return fail("no input pointers and no staged batch (cetkmc_stage_inputs)");
        if (g.step0 != a->step0 || g.n_steps != n || g.np_cap != a->np_cap || g.n_q != a->n_q || g.thermal_mode != a->thermal_mode ||
            (a->defect_fraction > 0.0 && !g.has_defect))
            return fail("the staged batch (cetkmc_stage_inputs) does not match this call's step0 / n_steps / np_cap / n_q / thermal_mode");
    }
    HIPCHK(hipSetDevice(h->dev));
    return staged ? 0 : upload_run_inputs(h, a);
}

// cetkmc_run_steps, part 2: the n steps queued on the stream.  therm_skip_g: the global step whose temperature update the
// previous (stopped) batch has already applied, or -1.  *q_idx: source planes handed to updates.
static int enqueue_steps(Handle* h, const cetkmc_run_args* a, const BatchCfg& cfg, ProfEvents& pe, int64_t therm_skip_g,
                         cetkmc_run_result* res, int64_t* q_idx)
{
    const int64_t n = a->n_steps;
    const bool incr = a->incremental && h->sweep_variant >= 1;
    // the apply kernel re-evaluates the <= 30 listed voxels an event touches, which keeps every listed voxel's sum
    // current between temperature updates (the interface kernel then runs only after one); off: the interface kernel
    // re-evaluates the whole list before every full sweep
    const int eval_touched = (h->sweep_variant >= 1 && !h->ifc_every_step) ? 1 : 0;
    // apply_in_sweep: a full-sweep step whose successor is no temperature-update step launches its selection alone; the next
    // sweep launch (the streaming kernel with the rate table, one slab, one process) applies the event.  The last step of the
    // call stays immediate, so no event is pending when the call returns.
    const bool pend_ok = h->apply_in_sweep && !incr && eval_touched && !multi_rank(h) && h->slabs.size() == 1 &&
                         h->sweep_variant == 1 && !(h->sweep_auto && h->L <= 128) && row_shape(h).hw;
    h->pend_live = false;
    h->pend_cfg = cfg;
    for (int64_t s = 0; s < n; ++s) {
        const int64_t g = a->step0 + s;
        const bool therm_due = a->thermal_mode && g % 20 == 0;
        const bool therm = therm_due && !(s == 0 && g == therm_skip_g);
        if (therm_due && !therm && a->thermal_mode == 2) ++*q_idx;      // its source plane was consumed by the stopped batch
        if (incr && s > 0 && !therm) {
            // exact incremental step: rates can only have changed in the rows recorded by the last apply
            ++h->cnt.incremental_steps;
            CHK(pe.record(s, 2));
            CHK(launch_dirty_rows(h, pe.pair(s, 0), pe.sweep(s, 1)));
            CHK(pe.record(s, 4));
            CHK(launch_select_apply(h, cfg, 1, h->d_dirty, s));
            invalidate(h, Cause::step);
            CHK(pe.record(s, 5));
            continue;
        }
        ++res->full_sweeps;
        if (pe.mode == 2) pe.was_full[s] = 1;
        CHK(pe.record(s, 0));
        if (therm) {
            CHK(batch_thermal(h, g, a->step0 + n, a->thermal_mode, a->thermal_dt, a->use_latent, q_idx));
            // remelting: behind the update and its prev_state := state, in front of this step's table / interface / sweep (no
            // event is pending here: a step before an update step is never deferred); the touched voxels are relisted and the
            // interface kernel, which follows every update, evaluates them
            if (h->ts.remelt_on) { CHK(launch_melt(h, h->ts.remelt_threshold, true)); invalidate(h, Cause::apply); }
            if (pe.mode == 2) pe.was_thermal[s] = 1;
        }
        const int rc_sw = launch_sweep(h, true, pe.sweep(s, 0), pe.sweep(s, 1), false, pe.phase(s, 1), pe.phase(s, 4));
        h->pend_live = false;
        CHK(rc_sw);
        if (pend_ok && s + 1 < n && !(a->thermal_mode && (g + 1) % 20 == 0)) {
            CHK(launch_select_pend(h, cfg, s));
            h->pend_live = true;
            ++h->cnt.deferred_steps;
        } else {
            CHK(launch_select_apply(h, cfg, (incr || eval_touched) ? 1 : 0, incr ? h->d_dirty : nullptr, s));
        }
        invalidate(h, (incr || eval_touched) ? Cause::step : Cause::step_no_upkeep);
        CHK(pe.record(s, 5));
    }
    return 0;
}

// cetkmc_run_steps, part 3: everything the host wants back travels behind ONE synchronisation -- step state, the per-step
// logs (all n entries; only the first steps_done are meaningful) and the interface lists' lengths
static int download_run(Handle* h, int64_t n, StepState* ss, double* totals, cetkmc_event* events, int64_t* n_events)
{
    const size_t nsl = h->slabs.size();
    const size_t o_tot = 64, o_ev = o_tot + (size_t)n * 8, o_nev = o_ev + (size_t)n * sizeof(cetkmc_event), o_len = o_nev + (size_t)n * 8;
    const size_t o_melt = (o_len + nsl * sizeof(int) + 7) & ~(size_t)7;        // the remelt counters, if the handle has any
    static_assert(sizeof(StepState) <= 64, "StepState grew: move the log offsets");
    CHK(grow_pinned(&h->pin_out, &h->pin_out_cap, o_melt + (h->ts.remelt_on ? 4 * 8 : 0)));
    const bool melt_read = h->ts.remelt_on && h->d_melt_block;      // only a loop that may have run a pass reads the counters
    if (melt_read) HIPCHK(hipMemcpyAsync(h->pin_out + o_melt, h->melt.cnt, 4 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->pin_out, h->d_ss, sizeof *ss, hipMemcpyDeviceToHost, h->stream));
    if (totals && n > 0) HIPCHK(hipMemcpyAsync(h->pin_out + o_tot, h->d_log_total, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    if (events && n > 0) HIPCHK(hipMemcpyAsync(h->pin_out + o_ev, h->d_log_event, (size_t)n * sizeof(cetkmc_event), hipMemcpyDeviceToHost, h->stream));
    if (n_events && n > 0) HIPCHK(hipMemcpyAsync(h->pin_out + o_nev, h->d_log_nev, (size_t)n * 8, hipMemcpyDeviceToHost, h->stream));
    for (size_t sl = 0; sl < nsl; ++sl)
        HIPCHK(hipMemcpyAsync(h->pin_out + o_len + sl * sizeof(int), h->slabs[sl].v.ifc_n, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    memcpy(ss, h->pin_out, sizeof *ss);
    if (melt_read) melt_info_from(h, (const unsigned long long*)(h->pin_out + o_melt));
    if (totals && n > 0) memcpy(totals, h->pin_out + o_tot, (size_t)n * 8);
    if (events && n > 0) memcpy(events, h->pin_out + o_ev, (size_t)n * sizeof(cetkmc_event));
    if (n_events && n > 0) memcpy(n_events, h->pin_out + o_nev, (size_t)n * 8);
    for (size_t sl = 0; sl < nsl; ++sl) {
        int n_list = 0;
        memcpy(&n_list, h->pin_out + o_len + sl * sizeof(int), sizeof(int));
        grow_ifc_grid(h, n_list);
    }
    h->cnt.bytes_d2h += (totals ? n * 8 : 0) + (events ? n * (int64_t)sizeof(cetkmc_event) : 0) + (n_events ? n * 8 : 0);
    return 0;
}

// The end of a stepping call, behind its synchronisation, with the step state it left (cetkmc_run_steps: its arguments and the
// marker it took; cetkmc_run_supersteps: neither).  A look-ahead never outlives its batch; a batch that stopped early leaves
// no cache (Cause::batch_stopped).  Mode A, stream exhausted (status 2) ON a temperature-update step: the continuation starts
// at that step and must not apply its update a second time (Handle::therm_applied_g).
static int end_batch(Handle* h, const StepState& ss, const cetkmc_run_args* a = nullptr, int64_t therm_skip_g = -1)
{
    if (h->spec.valid) { HIPCHK(hipStreamSynchronize(h->stream2)); h->spec.valid = false; }
    if (ss.status != 0) invalidate(h, Cause::batch_stopped);
    if (a && ss.status == 2) {
        const int64_t done = ss.cur, g = a->step0 + done;
        if (done == 0 && a->step0 == therm_skip_g)
            h->therm_applied_g = therm_skip_g;             // still the same pending step (nothing executed, nothing updated)
        else if (a->thermal_mode && done < a->n_steps && g % 20 == 0)
            h->therm_applied_g = g;                        // that step's update ran before the shortage was noticed
    }
    return 0;
}

int cetkmc_run_steps(void* handle, const cetkmc_run_args* a, cetkmc_run_result* res, double* totals,
                     cetkmc_event* events, int64_t* n_events)
{
    Handle* h = (Handle*)handle;
    if (!h || !a || !res) return fail("null argument");
    if (h->in_ensemble) return fail("an ensemble replica is stepped by cetkmc_run_ensemble");
    const int64_t n = a->n_steps;
    CHK(origin_room(h, n, "cetkmc_run_steps"));
    if (h->ts.bc_on && a->thermal_mode) CHK(boundary_steps_ok("cetkmc_run_steps", h->ts.bc, a->step0, n));
    if (h->ts.beam.on && a->thermal_mode == 2) CHK(beam_args_ok("cetkmc_run_steps", h->ts.beam, a->q_planes, a->n_q, a->step0, n));
    CHK(stage_run(h, a));
    // reset the batch part of the step state (nucleation_count persists): a one-thread kernel, no host round trip
    hipLaunchKernelGGL(k_batch_reset, dim3(1), dim3(1), 0, h->stream, h->d_ss);
    BatchCfg cfg{};
    cfg.step0 = a->step0; cfg.np_cap = a->np_cap; cfg.defect_fraction = a->defect_fraction; cfg.seed = a->seed;
    cfg.rng_mode = a->rng_mode; cfg.batch = 1;
    if (a->rng_mode == 2) cfg.np_cap = INT64_MAX / 2;       // no stream to run out of
    ProfEvents pe(h, a->profile, n);
    CHK(reserve_events(h, pe.needed()));
    h->time_comm = a->profile == 2 && multi_rank(h);
    h->comm_ev_used = 0;
    // continuation of a batch that ran out of stream on a temperature-update step: that update is already in the field
    const int64_t therm_skip_g = h->therm_applied_g;
    invalidate(h, Cause::marker_taken);
    int64_t q_idx = 0;
    res->full_sweeps = 0;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    CHK(enqueue_steps(h, a, cfg, pe, therm_skip_g, res, &q_idx));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    StepState ss;
    CHK(download_run(h, n, &ss, totals, events, n_events));
    CHK(end_batch(h, ss, a, therm_skip_g));
    CHK(origin_absorb_log(h, h->d_log_event, ss.cur, 1));      // the executed steps' events join the origin map
    if (h->time_comm) {
        for (size_t q = 0; q + 1 < h->comm_ev_used; q += 2) {
            CHK(add_elapsed(h->comm_ev[q], h->comm_ev[q + 1], &h->cnt.ms_comm));
            ++h->cnt.comm_calls;
        }
        h->time_comm = false; h->comm_ev_used = 0;
    }
    const int64_t done = ss.cur;
    res->steps_done = done; res->status = ss.status; res->np_used = ss.np_pos; res->q_used = q_idx;
    // q_idx counts the planes of every update the host queued; behind an early stop those updates ran as pass-throughs
    // and read no plane.  Consumed: the updates of the executed steps and of the step the batch stopped in (its update
    // precedes the selection that noticed the stop).
    if (ss.status != 0 && a->thermal_mode == 2) res->q_used = updates_in(a->step0, std::min(done + 1, n));
    res->nucleation_count = ss.nuc_count; res->min_margin = ss.min_margin;
    res->wall_ms = 0.0; res->sweep_ms_total = 0.0; res->sweep_launches = 0;
    CHK(add_elapsed(h->ev0, h->ev1, &res->wall_ms));
    CHK(pe.collect(res));
    h->cnt.steps += done;
    if (totals && ss.status == 1 && done < n) totals[done] = ss.total;
    return 0;
}

int cetkmc_get_counters(void* handle, cetkmc_counters* out, int reset)
{
    Handle* h = (Handle*)handle;
    if (!h || !out) return fail("null argument");
    *out = h->cnt;
    if (reset) h->cnt = cetkmc_counters{};
    return 0;
}

// ---- Mode B: synchronous super-steps over spatial boxes (superstep.hpp) ------------------------------
// kmc_simulation.py:331-332 per executed event of super-step g (DESIGN.md "Mode B": time advance; oracle orc_run_supersteps)
static double superstep_dt_event(uint64_t seed, int64_t g, double total)
{
    const double u = counter_uniform(seed, (uint64_t)g, KEY_DT);
    const double um = (u > 1e-12) ? u : 1e-12;              // max(1e-12, u)
    const double dt = -std::log(um) / total;
    return (1e-12 > dt) ? 1e-12 : dt;                       // max(dt, 1e-12)
}

// What the two Mode B drivers share (cetkmc_run_supersteps with box < L, cetkmc_run_supersteps_local): the batch of n
// super-steps over this handle's D boxes, NR log records per super-step.  super_begin readies the buffers and the step
// state, super_step_head issues a super-step up to the selection's totals, super_end closes the batch and hands the logs
// out; between head and end a driver issues its own pick / apply / exchange / touch / commit launches.  A new Mode B
// variant is a third driver of this shape.
struct SuperBatch {
    int64_t n = 0;
    int D = 0;
    size_t NR = 0;
    int thermal_mode = 0, use_latent = 0;
    double thermal_dt = 0.0;
    SuperCfg C{};
    BatchCfg cfg{};
    double* d_rmax = nullptr;
    cetkmc_event *d_dom = nullptr, *d_log = nullptr;
    DomPick* d_picks = nullptr;
    unsigned long long* d_cnt = nullptr;
};

// n_dom records of d_dom (dom_fill: set to type -1, nothing received); the log is kept for the caller's `events` and for an
// origin map; n_therm source planes from q_planes (thermal_mode 2)
static int super_begin(Handle* h, SuperBatch& B, size_t n_dom, bool dom_fill, bool want_events, const double* q_planes, int64_t n_therm)
{
    const size_t L2 = (size_t)h->L * h->L, n_rmax = (size_t)std::max(B.C.nranks, 1);
    invalidate(h, Cause::batch_begin);      // the batch buffers are reused below
    CHK(reserve_steps(h, (size_t)B.n));
    if (B.thermal_mode == 2) CHK(grow(&h->d_q, &h->cap_q, (size_t)std::max<int64_t>(n_therm, 1) * L2));
    // working buffers of the handle (grow-only; the previous call ended with a synchronisation, nothing still reads them)
    CHK(grow(&h->d_sup_rmax, &h->cap_sup_rmax, n_rmax));
    CHK(grow(&h->d_sup_dom, &h->cap_sup_dom, n_dom));
    CHK(grow(&h->d_sup_picks, &h->cap_sup_picks, (size_t)B.D));
    CHK(grow(&h->d_sup_cnt, &h->cap_sup_cnt, (size_t)SUPER_CNT_SLOTS * SUPER_CNT_STRIDE));
    const bool keep_log = (want_events || h->origin_on) && B.n > 0;      // an origin map reads the log on the device
    if (keep_log) CHK(grow(&h->d_sup_log, &h->cap_sup_log, (size_t)B.n * B.NR));
    B.d_rmax = h->d_sup_rmax; B.d_dom = h->d_sup_dom; B.d_picks = h->d_sup_picks; B.d_cnt = h->d_sup_cnt;
    B.d_log = keep_log ? h->d_sup_log : nullptr;
    HIPCHK(hipMemsetAsync(B.d_rmax, 0, n_rmax * sizeof(double), h->stream));
    if (dom_fill) HIPCHK(hipMemsetAsync(B.d_dom, 0xFF, n_dom * sizeof(cetkmc_event), h->stream));
    HIPCHK(hipMemsetAsync(B.d_cnt, 0, (size_t)SUPER_CNT_SLOTS * SUPER_CNT_STRIDE * sizeof(unsigned long long), h->stream));
    if (B.thermal_mode == 2 && n_therm > 0)
        HIPCHK(hipMemcpyAsync(h->d_q, q_planes, (size_t)n_therm * L2 * 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_batch_reset, dim3(1), dim3(1), 0, h->stream, h->d_ss);     // the batch part of the step state, on the stream
    B.cfg.step0 = B.C.step0; B.cfg.np_cap = 0; B.cfg.defect_fraction = B.C.defect_fraction; B.cfg.seed = B.C.seed;
    B.cfg.rng_mode = 1; B.cfg.batch = 1;
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    return 0;
}

// super-step s up to its selection: temperature update, interface list, sweep, total / counts / termination test
static int super_step_head(Handle* h, const SuperBatch& B, int64_t s, int64_t* q_idx)
{
    const int64_t g = B.C.step0 + s;
    if (B.thermal_mode && g % 20 == 0) CHK(batch_thermal(h, g, B.C.step0 + B.n, B.thermal_mode, B.thermal_dt, B.use_latent, q_idx));
    // interface sums: the list kernel after a temperature update / when something else made them stale (list
    // rebuilt in address order first: k_domain_touch flags new interface voxels without appending them); otherwise
    // they are current -- k_domain_touch re-evaluated what the events changed
    if (s > 0 && (!h->table_fresh || !h->ifc_fresh)) CHK(relist(h));
    CHK(launch_sweep(h, true, nullptr, nullptr, true));
    CHK(launch_select(h, B.cfg, 0.0, 1));
    return 0;
}

// the batch closed: result, origin map, per-super-step logs; *done = super-steps executed (for a driver's own logs)
static int super_end(Handle* h, const SuperBatch& B, int64_t q_used, cetkmc_run_result* res, double* totals, cetkmc_event* events,
                     int64_t* n_executed, double* dt_event, int64_t* done_out)
{
    StepState ss;
    if (B.n > 0) CHK(relist(h));        // leave a complete, address-ordered interface list behind (Mode A reads it)
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipMemcpyAsync(&ss, h->d_ss, sizeof ss, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    CHK(end_batch(h, ss));
    CHK(origin_absorb_log(h, B.d_log, ss.cur * (int64_t)B.NR, (int64_t)B.NR));      // every record of super-step t under the ordinal seq + t
    res->steps_done = ss.cur; res->status = ss.status; res->np_used = 0; res->q_used = q_used;
    res->nucleation_count = ss.nuc_count;
    res->wall_ms = 0.0;
    CHK(add_elapsed(h->ev0, h->ev1, &res->wall_ms));
    res->sweep_ms_total = 0.0; res->sweep_launches = 0; res->full_sweeps = B.n; res->min_margin = 1.0;
    h->cnt.supersteps += ss.cur;
    CHK(refresh_ifc_grid(h));
    const int64_t done = *done_out = ss.cur;
    if ((totals || dt_event) && done > 0) {
        std::vector<double> tot((size_t)done);
        HIPCHK(hipMemcpy(tot.data(), h->d_log_total, (size_t)done * 8, hipMemcpyDeviceToHost));
        if (totals) memcpy(totals, tot.data(), (size_t)done * 8);
        if (dt_event) for (int64_t s = 0; s < done; ++s) dt_event[s] = superstep_dt_event(B.C.seed, B.C.step0 + s, tot[(size_t)s]);
    }
    if (totals && ss.status == 1 && done < B.n) totals[done] = ss.total;
    if (n_executed && done > 0) HIPCHK(hipMemcpy(n_executed, h->d_log_nev, (size_t)done * 8, hipMemcpyDeviceToHost));
    if (events && done > 0) HIPCHK(hipMemcpy(events, B.d_log, (size_t)done * B.NR * sizeof(cetkmc_event), hipMemcpyDeviceToHost));
    return 0;
}

int cetkmc_run_supersteps(void* handle, const cetkmc_super_args* a, cetkmc_run_result* res, double* totals,
                          cetkmc_event* events, int64_t* n_executed, double* dt_event)
{
    Handle* h = (Handle*)handle;
    if (!h || !a || !res) return fail("null argument");
    if (h->in_ensemble) return fail("an ensemble replica is stepped by cetkmc_run_ensemble");
    CHK(thermal_exclusions(h->ts, "cetkmc_run_supersteps"));
    const int64_t n = a->n_steps;
    if (n < 0) return fail("n_steps < 0");
    if (h->sweep_variant < 1) return fail("cetkmc_run_supersteps needs a streaming sweep_variant (1 or 2)");
    if (a->box == h->L) {
        // single domain (window = whole lattice, no octants): one event per super-step from the global canonical tree --
        // this IS a Mode A step whose uniforms are the counter-based ones of box 0, so it runs through the Mode A kernels
        if (multi_rank(h) && h->nranks > 1) return fail("the single-domain case (box == L) runs in one process");
        cetkmc_run_args ra{};
        ra.step0 = a->step0; ra.n_steps = n; ra.defect_fraction = a->defect_fraction;
        ra.rng_mode = 2; ra.seed = a->seed; ra.thermal_mode = a->thermal_mode; ra.thermal_dt = a->thermal_dt;
        ra.q_planes = a->q_planes; ra.n_q = a->n_q; ra.use_latent = a->use_latent;
        std::vector<double> tot((size_t)n + 1, 0.0);
        CHK(cetkmc_run_steps(handle, &ra, res, tot.data(), events, nullptr));
        const int64_t done = res->steps_done;
        for (int64_t s = 0; s < done; ++s) {
            if (totals) totals[s] = tot[(size_t)s];
            if (n_executed) n_executed[s] = 1;
            if (dt_event) dt_event[s] = superstep_dt_event(a->seed, a->step0 + s, tot[(size_t)s]);
        }
        if (totals && res->status == 1 && done < n) totals[done] = tot[(size_t)done];
        h->cnt.supersteps += done;
        return 0;
    }
    if (a->box < 8 || a->box > 16 || (a->box & 1) || h->L % a->box) return fail("box must be even, 8..16, and divide L (or equal L: single domain)");
    const bool ranks = multi_rank(h) && h->nranks > 1;
    if (ranks && h->nranks > 64) return fail("Mode B supports up to 64 ranks");
    if (ranks && (h->L / h->nranks) % a->box) return fail("across ranks the boxes must be aligned to the slabs: (L / nranks) % box == 0");
    const int64_t n_therm = a->thermal_mode ? updates_in(a->step0, n) : 0;
    if (a->thermal_mode == 2 && (n_therm > a->n_q || (n_therm > 0 && !a->q_planes)))
        return fail("thermal_mode 2 needs one q plane per thermal update in the batch");
    CHK(origin_room(h, n, "cetkmc_run_supersteps"));
    HIPCHK(hipSetDevice(h->dev));
    SuperBatch B;
    B.n = n; B.thermal_mode = a->thermal_mode; B.thermal_dt = a->thermal_dt; B.use_latent = a->use_latent;
    SuperCfg& C = B.C;
    C.step0 = a->step0; C.defect_fraction = a->defect_fraction; C.seed = a->seed;
    C.box = a->box; C.H = a->box / 2; C.nb = h->L / a->box;
    C.PH = 1; while (C.PH < C.H) C.PH <<= 1;
    C.PT = 1; while (C.PT < 3 * C.H) C.PT <<= 1;
    // this handle's boxes: the box layers of its owned planes (all of them in a single process); global box index
    // d = (di * nb + dj) * nb + dk, so they are the contiguous range [d0, d0 + D)
    const int nb2 = C.nb * C.nb;
    C.d0 = ranks ? (h->own_i0 / a->box) * nb2 : 0;
    const int D = ranks ? ((h->own_i1 - h->own_i0) / a->box) * nb2 : C.nb * nb2;
    C.D_loc = D;
    C.null_events = a->null_events ? 1 : 0;
    C.nranks = ranks ? h->nranks : 1;
    B.D = D; B.NR = (size_t)D;
    const int NE = D + 2 * nb2;                               // own events | lower neighbour's top layer | upper neighbour's bottom layer
    const size_t shmem = (size_t)C.PT * C.PH * C.PH * 19;     // heap: 2*NL doubles + 2*NL flags, NL leaf codes
    CHK(super_begin(h, B, (size_t)NE, true, events != nullptr, a->q_planes, n_therm));
    double* const d_rmax = B.d_rmax;
    cetkmc_event* const d_dom = B.d_dom;
    DomPick* const d_picks = B.d_picks;
    int64_t q_idx = 0;
    for (int64_t s = 0; s < n; ++s) {
        CHK(super_step_head(h, B, s, &q_idx));
        if (C.H == 4)       // box 8: window tree in registers
            hipLaunchKernelGGL(k_domain_pick8, dim3(D), dim3(64), 0, h->stream, h->kp, (const SlabView*)dviews(h),
                               (int)h->slabs.size(), h->L, C, (const StepState*)h->d_ss, (const double*)h->d_ktab, d_picks, (long long)s);
        else
            hipLaunchKernelGGL(k_domain_pick, dim3(D), dim3(64), shmem, h->stream, h->kp, (const SlabView*)dviews(h),
                               (int)h->slabs.size(), h->L, C, (const StepState*)h->d_ss, (const double*)h->d_ktab, d_picks);
        if (C.null_events) {
            // R_max of the super-step: this rank's largest window total, then (across ranks) the largest of all ranks
            hipLaunchKernelGGL(k_domain_rmax, dim3((D + 1023) / 1024), dim3(1024), 0, h->stream, (const DomPick*)d_picks, D, (const StepState*)h->d_ss,
                               d_rmax, ranks ? h->rank : 0);
            if (ranks) CHK(comm_allgather(h, d_rmax, sizeof(double)));
        }
        hipLaunchKernelGGL(k_domain_apply, dim3((D + 63) / 64), dim3(64), 0, h->stream, h->kp, (const SlabView*)dviews(h),
                           (int)h->slabs.size(), h->L, D, C, h->d_ss, (const DomPick*)d_picks, d_dom, B.d_cnt, B.d_log, (const double*)d_rmax);
        int n_touch = D;
        if (ranks) {
            // the events of my bottom / top box layer go to the ranks below / above, theirs come here: every rank applies
            // them to its own copy (owned planes: diffusion targets across the boundary; halo planes: the neighbour's state)
            CHK(comm_exchange(h, d_dom, d_dom + D, d_dom + (D - nb2), d_dom + D + nb2, (size_t)nb2 * sizeof(cetkmc_event)));
            hipLaunchKernelGGL(k_domain_apply_remote, dim3((2 * nb2 + 63) / 64), dim3(64), 0, h->stream, (const SlabView*)dviews(h),
                               (int)h->slabs.size(), C, (const StepState*)h->d_ss, (const cetkmc_event*)(d_dom + D));
            n_touch = NE;
        }
        hipLaunchKernelGGL(k_domain_touch, dim3(2 * ((n_touch + 15) / 16)), dim3(256), 0, h->stream, h->kp, (const SlabView*)dviews(h),
                           (int)h->slabs.size(), n_touch, (const cetkmc_event*)d_dom, (const StepState*)h->d_ss, (const double*)h->d_ktab);
        hipLaunchKernelGGL(k_super_commit, dim3(1), dim3(64), 0, h->stream, h->d_ss, B.d_cnt, h->d_log_total, h->d_log_nev,
                           C.null_events ? d_rmax : (double*)nullptr, std::min(C.nranks, 64));
        invalidate(h, Cause::step);      // (k_domain_touch re-evaluated the listed voxels the events changed)
    }
    int64_t done = 0;
    return super_end(h, B, q_idx, res, totals, events, n_executed, dt_event, &done);
}

// ---- Mode B with a local event loop (local.hpp) ------------------------------------------------------
int cetkmc_run_supersteps_local(void* handle, const cetkmc_local_args* a, cetkmc_run_result* res, double* totals,
                                cetkmc_event* events, int64_t* n_executed, double* dt_event, double* horizon, int64_t* n_capped)
{
    Handle* h = (Handle*)handle;
    if (!h || !a || !res) return fail("null argument");
    if (h->in_ensemble) return fail("an ensemble replica is stepped by cetkmc_run_ensemble");
    CHK(thermal_exclusions(h->ts, "cetkmc_run_supersteps_local"));
    const int64_t n = a->n_steps;
    if (n < 0) return fail("n_steps < 0");
    if (a->box != 8 || h->L % 8) return fail("cetkmc_run_supersteps_local: box must be 8 and divide L");
    if (a->max_events < 1 || a->max_events > 64) return fail("cetkmc_run_supersteps_local: max_events must be 1..64");
    if (!(a->horizon_events > 0.0)) return fail("cetkmc_run_supersteps_local: horizon_events must be > 0 (it may be +inf)");
    if (a->thermal_mode == 2) return fail("cetkmc_run_supersteps_local: thermal_mode 2 (laser) is not supported in this mode");
    if (a->thermal_mode != 0 && a->thermal_mode != 1) return fail("cetkmc_run_supersteps_local: thermal_mode must be 0 or 1");
    CHK(one_slab_only(h, "cetkmc_run_supersteps_local", ""));
    if (h->sweep_variant < 1) return fail("cetkmc_run_supersteps_local needs a streaming sweep_variant (1 or 2)");
    CHK(origin_room(h, n, "cetkmc_run_supersteps_local"));
    HIPCHK(hipSetDevice(h->dev));
    SuperBatch B;
    B.n = n; B.thermal_mode = a->thermal_mode; B.thermal_dt = a->thermal_dt;
    SuperCfg& C = B.C;
    C.step0 = a->step0; C.defect_fraction = a->defect_fraction; C.seed = a->seed;
    C.box = 8; C.H = 4; C.PH = 4; C.PT = 16; C.nb = h->L / 8;
    const int D = C.nb * C.nb * C.nb, K = a->max_events;
    C.d0 = 0; C.D_loc = D; C.null_events = 0; C.nranks = 1;
    LocalCfg LC{};
    LC.max_events = K; LC.horizon_events = a->horizon_events;
    const size_t NR = (size_t)D * K;                              // records per super-step
    B.D = D; B.NR = NR;
    CHK(grow(&h->d_loc_horizon, &h->cap_loc_horizon, (size_t)std::max<int64_t>(n, 1)));
    CHK(grow(&h->d_loc_capped, &h->cap_loc_capped, (size_t)std::max<int64_t>(n, 1)));
    CHK(super_begin(h, B, NR, false, events != nullptr, nullptr, 0));
    double* const d_rmax = B.d_rmax;
    int64_t q_idx = 0;
    for (int64_t s = 0; s < n; ++s) {
        CHK(super_step_head(h, B, s, &q_idx));
        const SlabView* views = (const SlabView*)dviews(h);
        hipLaunchKernelGGL(k_domain_pick8, dim3(D), dim3(64), 0, h->stream, h->kp, views, 1, h->L, C, (const StepState*)h->d_ss,
                           (const double*)h->d_ktab, B.d_picks, (long long)s);
        hipLaunchKernelGGL(k_domain_rmax, dim3((D + 1023) / 1024), dim3(1024), 0, h->stream, (const DomPick*)B.d_picks, D, (const StepState*)h->d_ss,
                           d_rmax, 0);
        hipLaunchKernelGGL(k_domain_local, dim3(D), dim3(64), 0, h->stream, h->kp, views, h->L, D, C, LC, (const StepState*)h->d_ss,
                           (const double*)h->d_ktab, (const DomPick*)B.d_picks, (const double*)d_rmax, B.d_dom, B.d_cnt, B.d_log);
        // upkeep of everything touched, after all lattice writes of the super-step (evaluates the lattice as it stands now:
        // several records of one neighbourhood give the same result)
        hipLaunchKernelGGL(k_domain_touch, dim3(2 * (unsigned)((NR + 15) / 16)), dim3(256), 0, h->stream, h->kp, views, 1, (int)NR,
                           (const cetkmc_event*)B.d_dom, (const StepState*)h->d_ss, (const double*)h->d_ktab);
        hipLaunchKernelGGL(k_local_commit, dim3(1), dim3(64), 0, h->stream, (const StepState*)h->d_ss, B.d_cnt, (const double*)d_rmax, LC,
                           h->d_loc_horizon, h->d_loc_capped);
        hipLaunchKernelGGL(k_super_commit, dim3(1), dim3(64), 0, h->stream, h->d_ss, B.d_cnt, h->d_log_total, h->d_log_nev, d_rmax, 1);
        invalidate(h, Cause::step);
    }
    int64_t done = 0;
    CHK(super_end(h, B, q_idx, res, totals, events, n_executed, dt_event, &done));
    if (horizon && done > 0) HIPCHK(hipMemcpy(horizon, h->d_loc_horizon, (size_t)done * 8, hipMemcpyDeviceToHost));
    if (n_capped && done > 0) HIPCHK(hipMemcpy(n_capped, h->d_loc_capped, (size_t)done * 8, hipMemcpyDeviceToHost));
    return 0;
}

// ---- grain clustering (utils.get_clusters / dfs_cluster, utils.py:28-84) ---------------------------
// the per-voxel arrays of a handle's clustering (all at once: d_cc_parent stands for the five)
static int cc_alloc(Handle* h)
{
    if (h->d_cc_parent) return 0;
    const int64_t n = (int64_t)h->L * h->L * h->L;
    HIPCHK(hipMalloc((void**)&h->d_cc_parent, n * sizeof(int)));
    HIPCHK(hipMalloc((void**)&h->d_cc_roots, n * sizeof(int)));
    HIPCHK(hipMalloc((void**)&h->d_cc_cid, n * sizeof(int)));
    HIPCHK(hipMalloc((void**)&h->d_cc_labels, n * sizeof(int)));
    HIPCHK(hipMalloc((void**)&h->d_cc_n, sizeof(int)));
    return 0;
}

int cetkmc_cluster(void* handle, double threshold, int64_t* n_clusters)
{
    Handle* h = (Handle*)handle;
    if (!h || !n_clusters) return fail("null argument");
    if (h->slabs.size() != 1 || h->nranks != 1) return fail("cetkmc_cluster needs the whole lattice in one slab");
    HIPCHK(hipSetDevice(h->dev));
    const SlabView v = view_of(h, 0);
    const int64_t n = (int64_t)h->L * h->L * h->L;
    CHK(cc_alloc(h));
    const int grid = (int)std::min<int64_t>((n + 255) / 256, 8192);
    HIPCHK(hipMemsetAsync(h->d_cc_n, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_cc_init, dim3(grid), dim3(256), 0, h->stream, v, h->d_cc_parent);
    hipLaunchKernelGGL(k_cc_hook, dim3(grid), dim3(256), 0, h->stream, v, h->d_cc_parent, threshold);
    hipLaunchKernelGGL(k_cc_compress, dim3(grid), dim3(256), 0, h->stream, n, h->d_cc_parent, h->d_cc_roots, h->d_cc_n);
    HIPCHK(hipGetLastError());
    int nr = 0;
    HIPCHK(hipMemcpyAsync(&nr, h->d_cc_n, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cc_roots_sorted.resize((size_t)nr);
    if (nr > 0) {
        HIPCHK(hipMemcpy(h->cc_roots_sorted.data(), h->d_cc_roots, (size_t)nr * sizeof(int), hipMemcpyDeviceToHost));
        std::sort(h->cc_roots_sorted.begin(), h->cc_roots_sorted.end());      // reference order: first voxel, row-major
        HIPCHK(hipMemcpy(h->d_cc_roots, h->cc_roots_sorted.data(), (size_t)nr * sizeof(int), hipMemcpyHostToDevice));
        if (h->d_cc_stats) { HIPCHK(hipFree(h->d_cc_stats)); h->d_cc_stats = nullptr; }
        HIPCHK(hipMalloc((void**)&h->d_cc_stats, (size_t)nr * 8 * sizeof(int)));
        const int g2 = (nr + 255) / 256;
        hipLaunchKernelGGL(k_cc_ids, dim3(g2), dim3(256), 0, h->stream, (const int*)h->d_cc_roots, nr, h->d_cc_cid);
        hipLaunchKernelGGL(k_cc_stats_init, dim3(g2), dim3(256), 0, h->stream, nr, h->d_cc_stats);
    }
    hipLaunchKernelGGL(k_cc_stats, dim3(grid), dim3(256), 0, h->stream, v, (const int*)h->d_cc_parent, (const int*)h->d_cc_cid,
                       h->d_cc_labels, h->d_cc_stats);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cc_n_clusters = nr;
    *n_clusters = nr;
    return 0;
}

int cetkmc_cluster_stats(void* handle, int64_t cap, int32_t* first_voxel, int64_t* size, int32_t* bbox)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    if (h->cc_n_clusters < 0) return fail("cetkmc_cluster_stats needs a preceding cetkmc_cluster");
    const int64_t n = std::min<int64_t>(cap, h->cc_n_clusters);
    if (n <= 0) return 0;
    std::vector<int> st((size_t)n * 8);
    HIPCHK(hipMemcpy(st.data(), h->d_cc_stats, st.size() * sizeof(int), hipMemcpyDeviceToHost));
    const int L = h->L;
    for (int64_t q = 0; q < n; ++q) {
        const int r = h->cc_roots_sorted[(size_t)q];
        if (first_voxel) { first_voxel[3 * q] = r / (L * L); first_voxel[3 * q + 1] = (r / L) % L; first_voxel[3 * q + 2] = r % L; }
        if (size) size[q] = st[8 * q];
        if (bbox) for (int c = 0; c < 6; ++c) bbox[6 * q + c] = st[8 * q + 1 + c];
    }
    return 0;
}

int cetkmc_cluster_labels(void* handle, int32_t* labels)
{
    Handle* h = (Handle*)handle;
    if (!h || !labels) return fail("null argument");
    if (h->cc_n_clusters < 0) return fail("cetkmc_cluster_labels needs a preceding cetkmc_cluster");
    HIPCHK(hipMemcpy(labels, h->d_cc_labels, (size_t)h->L * h->L * h->L * sizeof(int), hipMemcpyDeviceToHost));
    return 0;
}

// ---- imported labellings -----------------------------------------------------------------------
// One host pass over a label volume of L^3 voxels: refuses anything but ids numbered 1, 2, .. by first occurrence in row-major
// order (0 = empty) -- so no label is negative or beyond n, every id 1..n is present and the roots come out ascending, which
// is what k_layer_profile's roots[g - 1] / eq[g] lookups and its n_start shortcut rely on -- and derives what cetkmc_cluster
// leaves behind: roots[id - 1] = linear index of the grain's first voxel, and k_cc_stats' table {size, min3, max3, 0}.
// `rep` < 0: a single lattice; otherwise the replica named in the message.
static int cc_import_scan(const char* who, const int32_t* lab, int L, int rep, std::vector<int>& roots, std::vector<int>& stats)
{
    const int64_t n = (int64_t)L * L * L;
    roots.clear(); stats.clear();
    for (int64_t x = 0; x < n; ++x) {
        const int g = lab[x];
        if (g == 0) continue;
        const int c[3] = {(int)(x / ((int64_t)L * L)), (int)((x / L) % L), (int)(x % L)};
        const int64_t seen = (int64_t)roots.size();
        if (g < 0 || g > seen + 1) {
            const std::string at = "label " + std::to_string(g) + " at voxel (" + std::to_string(c[0]) + ", " + std::to_string(c[1]) + ", " +
                                   std::to_string(c[2]) + ")" + (rep >= 0 ? " of replica " + std::to_string(rep) : std::string());
            return fail(std::string(who) + ": " + at + (g < 0 ? ": labels are 0 (empty) or ids 1..n"
                        : ": ids are numbered 1..n by first occurrence in row-major order, the next new id here is " + std::to_string(seen + 1)));
        }
        if (g == seen + 1) {
            roots.push_back((int)x);
            const int fresh[8] = {0, c[0], c[1], c[2], c[0], c[1], c[2], 0};
            stats.insert(stats.end(), fresh, fresh + 8);
        }
        int* s = &stats[(size_t)8 * (size_t)(g - 1)];
        s[0] += 1;
        for (int a = 0; a < 3; ++a) { s[1 + a] = std::min(s[1 + a], c[a]); s[4 + a] = std::max(s[4 + a], c[a]); }
    }
    return 0;
}

int cetkmc_cluster_import(void* handle, const int32_t* labels, int64_t* n_clusters)
{
    Handle* h = (Handle*)handle;
    if (!h || !labels || !n_clusters) return fail("null argument");
    if (ens_of(handle)) return fail("cetkmc_cluster_import takes one lattice: an ensemble handle goes to cetkmc_ensemble_cluster_import");
    if (h->slabs.size() != 1 || h->nranks != 1) return fail("cetkmc_cluster_import needs the whole lattice in one slab");
    std::vector<int> roots, stats;
    CHK(cc_import_scan("cetkmc_cluster_import", labels, h->L, -1, roots, stats));
    HIPCHK(hipSetDevice(h->dev));
    const int64_t n = (int64_t)h->L * h->L * h->L;
    const size_t nr = roots.size();
    CHK(cc_alloc(h));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (nr > 0) {
        if (h->d_cc_stats) { HIPCHK(hipFree(h->d_cc_stats)); h->d_cc_stats = nullptr; }
        HIPCHK(hipMalloc((void**)&h->d_cc_stats, nr * 8 * sizeof(int)));
        HIPCHK(hipMemcpyAsync(h->d_cc_roots, roots.data(), nr * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_cc_stats, stats.data(), nr * 8 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipMemcpyAsync(h->d_cc_labels, labels, (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cnt.bytes_h2d += (int64_t)(((size_t)n + nr * 9) * sizeof(int));
    h->cc_roots_sorted.swap(roots);
    h->cc_n_clusters = (int64_t)nr;
    *n_clusters = (int64_t)nr;
    return 0;
}

int cetkmc_species_counts(void* handle, int64_t counts[6])
{
    Handle* h = (Handle*)handle;
    if (!h || !counts) return fail("null argument");
    HIPCHK(hipSetDevice(h->dev));
    DevTmp<unsigned long long> d;
    HIPCHK(d.alloc(6));
    HIPCHK(hipMemsetAsync(d, 0, 6 * sizeof(unsigned long long), h->stream));
    for (size_t s = 0; s < h->slabs.size(); ++s)
        hipLaunchKernelGGL(k_species_counts, dim3(1024), dim3(256), 0, h->stream, view_of(h, (int)s), d.p);
    HIPCHK(hipGetLastError());
    unsigned long long out[6];
    HIPCHK(hipMemcpyAsync(out, d, sizeof out, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    for (int c = 0; c < 6; ++c) counts[c] = (int64_t)out[c];
    return 0;
}

int cetkmc_gather_species(void* handle, int species, int64_t* lin_idx, double* T_vals, int64_t cap, int64_t* n)
{
    Handle* h = (Handle*)handle;
    if (!h || !n) return fail("null argument");
    HIPCHK(hipSetDevice(h->dev));
    DevTmp<unsigned long long> d_n;
    DevTmp<long long> d_idx;
    DevTmp<double> d_T;
    const size_t c = (size_t)std::max<int64_t>(cap, 1);
    HIPCHK(d_n.alloc(1));
    HIPCHK(d_idx.alloc(c));
    HIPCHK(d_T.alloc(c));
    HIPCHK(hipMemsetAsync(d_n, 0, sizeof(unsigned long long), h->stream));
    for (size_t s = 0; s < h->slabs.size(); ++s)
        hipLaunchKernelGGL(k_gather_species, dim3(1024), dim3(256), 0, h->stream, view_of(h, (int)s), species, d_idx.p, d_T.p,
                           (unsigned long long)(lin_idx && T_vals ? cap : 0), d_n.p);
    HIPCHK(hipGetLastError());
    unsigned long long cnt = 0;
    HIPCHK(hipMemcpyAsync(&cnt, d_n, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *n = (int64_t)cnt;
    const size_t m = (size_t)std::min<int64_t>((int64_t)cnt, cap);
    if (lin_idx && T_vals && m > 0) {
        HIPCHK(hipMemcpy(lin_idx, d_idx, m * sizeof(long long), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(T_vals, d_T, m * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

int cetkmc_set_defects_sparse(void* handle, const int64_t* lin_idx, int64_t n)
{
    Handle* h = (Handle*)handle;
    if (!h || (n > 0 && !lin_idx)) return fail("null argument");
    HIPCHK(hipSetDevice(h->dev));
    DevTmp<long long> d_idx;
    if (n > 0) {
        HIPCHK(d_idx.alloc((size_t)n));
        HIPCHK(hipMemcpyAsync(d_idx, lin_idx, (size_t)n * sizeof(long long), hipMemcpyHostToDevice, h->stream));
    }
    for (auto& s : h->slabs) {
        HIPCHK(hipMemsetAsync(s.v.defects, 0, s.nS, h->stream));
        if (n > 0) hipLaunchKernelGGL(k_scatter_defects, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0,
                                      h->stream, s.v, (const long long*)d_idx.p, (long long)n);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    invalidate(h, Cause::set_defects);
    return 0;
}

int64_t cetkmc_nucleation_count(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return -1;
    StepState ss;
    if (hipSetDevice(h->dev) != hipSuccess) return -1;
    if (hipMemcpy(&ss, h->d_ss, sizeof ss, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return ss.nuc_count;
}

int cetkmc_reset_counters(void* handle)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipMemsetAsync(h->d_ss, 0, sizeof(StepState), h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

#ifdef CETKMC_SEL_STAMPS
int cetkmc_debug_sel_stamps(long long out[16])      /* alternative builds only (tools/sel_stamps.py); not part of the ABI */
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(cetkmc::g_sel_stamps), 16 * sizeof(long long)));
    return 0;
}
int cetkmc_debug_pend_stamps(unsigned long long out[8])     /* the apply block of k_sweep_stream_apply (tools/pend_stamps.py) */
{
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(out, HIP_SYMBOL(cetkmc::g_pend_stamps), 8 * sizeof(unsigned long long)));
    return 0;
}
#endif

int cetkmc_time_sweeps(void* handle, int n, double* ms_total)
{
    Handle* h = (Handle*)handle;
    if (!h || !ms_total) return fail("null argument");
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int s = 0; s < n; ++s) CHK(launch_sweep(h, false));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *ms_total = 0.0;
    return add_elapsed(h->ev0, h->ev1, ms_total);
}

int cetkmc_event_overhead(void* handle, int n, double* ms_avg)
{
    Handle* h = (Handle*)handle;
    if (!h || !ms_avg || n < 1) return fail("bad argument");
    HIPCHK(hipSetDevice(h->dev));
    CHK(reserve_events(h, 2 * n));
    for (int q = 0; q < n; ++q) {
        // a kernel before the pair as well: the bracketed launches of a batch follow other kernels back to back
        hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, h->stream);
        HIPCHK(hipEventRecord(h->prof[2 * q], h->stream));
        hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, h->stream);
        HIPCHK(hipEventRecord(h->prof[2 * q + 1], h->stream));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    double tot = 0.0;
    for (int q = 0; q < n; ++q) CHK(add_elapsed(h->prof[2 * q], h->prof[2 * q + 1], &tot));
    *ms_avg = tot / n;
    return 0;
}

// Transport self-test: every collective shape the stepping loops use, on patterned buffers, checked on the host.
//   all-gather of `bytes` per rank (Mode A: block sums / event records) and the neighbour exchange of `bytes` each way
//   (temperature halo, Mode B boundary layers).  A single-rank RCCL communicator sends to and receives from itself.
// times_us (optional, 2 doubles): average of 20 back-to-back all-gathers / exchanges after the checked one.
int cetkmc_comm_selftest(void* handle, int64_t bytes, double* times_us)
{
    Handle* h = (Handle*)handle;
    if (!h || bytes < 1 || bytes > (1 << 26)) return fail("bad argument");
    HIPCHK(hipSetDevice(h->dev));
    if (times_us) times_us[0] = times_us[1] = 0.0;
    if (!multi_rank(h)) return 0;
    const int R = h->nranks, me = h->rank;
    const size_t B = (size_t)bytes;
    auto pat = [](int from, int tag, size_t q) -> unsigned char { return (unsigned char)(from * 37 + tag * 101 + q * 7 + (q >> 8)); };
    char* d = nullptr;          // [gather: R*B | send_lo | send_hi | recv_lo | recv_hi]
    HIPCHK(hipMalloc(&d, (R + 4) * B));
    std::vector<unsigned char> host((R + 4) * B, 0xEE);
    for (size_t q = 0; q < B; ++q) {
        host[me * B + q] = pat(me, 0, q);
        host[(R + 0) * B + q] = pat(me, 1, q);      // to rank-1
        host[(R + 1) * B + q] = pat(me, 2, q);      // to rank+1
    }
    HIPCHK(hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice));
    int rc = comm_allgather(h, d, B);
    if (!rc) {
        if (h->comm && R == 1) {            // loopback: the Send/Recv signatures and group semantics on this build of RCCL
            NCCLCHK(g_rccl.GroupStart());
            NCCLCHK(g_rccl.Send(d + (R + 0) * B, B, ncclChar, 0, h->comm, h->stream));
            NCCLCHK(g_rccl.Recv(d + (R + 2) * B, B, ncclChar, 0, h->comm, h->stream));
            NCCLCHK(g_rccl.GroupEnd());
        } else {
            rc = comm_exchange(h, d + (R + 0) * B, d + (R + 2) * B, d + (R + 1) * B, d + (R + 3) * B, B);
        }
    }
    if (rc) { (void)hipFree(d); return rc; }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(host.data(), d, host.size(), hipMemcpyDeviceToHost));
    std::string bad;
    for (int r = 0; r < R && bad.empty(); ++r)
        for (size_t q = 0; q < B; ++q)
            if (host[r * B + q] != pat(r, 0, q)) { bad = "all-gather: part of rank " + std::to_string(r) + " wrong at byte " + std::to_string(q); break; }
    if (bad.empty() && h->comm && R == 1) {
        for (size_t q = 0; q < B; ++q) if (host[(R + 2) * B + q] != pat(0, 1, q)) { bad = "loopback send/recv wrong at byte " + std::to_string(q); break; }
    } else if (bad.empty()) {
        for (size_t q = 0; q < B && bad.empty(); ++q) {
            // from rank-1 comes what it sent "to rank+1" (tag 2); from rank+1 what it sent "to rank-1" (tag 1)
            if (me > 0 && host[(R + 2) * B + q] != pat(me - 1, 2, q)) bad = "exchange: data from rank-1 wrong at byte " + std::to_string(q);
            if (me < R - 1 && host[(R + 3) * B + q] != pat(me + 1, 1, q)) bad = "exchange: data from rank+1 wrong at byte " + std::to_string(q);
            if (me == 0 && host[(R + 2) * B + q] != 0xEE) bad = "exchange: end rank's unused receive buffer was written";
        }
    }
    if (!bad.empty()) { (void)hipFree(d); return fail("transport self-test (rank " + std::to_string(me) + "): " + bad); }
    if (times_us) {
        for (int leg = 0; leg < 2; ++leg) {
            HIPCHK(hipStreamSynchronize(h->stream));
            const auto t0 = std::chrono::steady_clock::now();
            for (int q = 0; q < 20 && !rc; ++q)
                rc = leg == 0 ? comm_allgather(h, d, B)
                              : comm_exchange(h, d + (R + 0) * B, d + (R + 2) * B, d + (R + 1) * B, d + (R + 3) * B, B);
            if (rc) { (void)hipFree(d); return rc; }
            HIPCHK(hipStreamSynchronize(h->stream));
            times_us[leg] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 20.0;
        }
    }
    HIPCHK(hipFree(d));
    return 0;
}

// ---- replica ensembles (ensemble.hpp) ----------------------------------------------------------
int cetkmc_create_ensemble(const cetkmc_params* p, int L, int R, int device_id, void** handle)
{
    if (!p || !handle) return fail("null argument");
    *handle = nullptr;
    if (R < 1) return fail("an ensemble needs R >= 1 replicas");
    if (L < 1 || L > 128) return fail("ensembles cover 1 <= L <= 128 (one lattice of L > 128 already fills the GPU)");
    {   // grid limits: the replica rides in y (z for the temperature march: z = replica x plane groups of THERM_NI planes)
        const int64_t nz = (L + THERM_NI - 1) / THERM_NI;
        if ((int64_t)R * nz > 65535) return fail("too many replicas for this L: R * ceil(L / " + std::to_string(THERM_NI) + ") must be <= 65535");
        // device memory: fields, tables and lists of a handle + the batched analysis arrays, against what is free now
        const int64_t L2 = (int64_t)L * L, RJ = round_up(L, SWEEP_TJ) + 4, pT = round_up(L, 8);
        const int64_t per = 3 * (L + 4) * RJ * round_up(KOFF + L + 4, 16) + (L + 4) * RJ * round_up(KOFFC + L + 12, 16) +
                            (L + 4) * L * pT * (8 * 10 + 1 + 4) + L2 * L * 4 + 2 * L2 * pT * 8 + L * 3 * L * 12 +
                            L2 * L * (4 * 4 + 16) + (1 << 20);
        size_t free_b = 0, total_b = 0;
        if (hipSetDevice(device_id) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
            (double)per * R > 0.9 * (double)free_b)
            return fail("ensemble does not fit in device memory: ~" + std::to_string((long long)(per * R >> 20)) + " MiB needed, " +
                        std::to_string((long long)(free_b >> 20)) + " MiB free");
    }
    Ens* e = new Ens();
    e->L = L; e->R = R;
    auto bail = [&](int rc) { destroy_ens(e); return rc; };
    for (int r = 1; r < R; ++r)
        if (!shared_params_equal(p[0], p[r])) return bail(fail(SHARED_PARAMS_MSG));
    const std::vector<std::pair<int, int>> ranges{{0, L}};
    for (int r = 0; r < R; ++r) {
        void* hv = nullptr;
        if (int rc = create_common(&p[r], L, ranges, device_id, 1, 0, &hv, r ? e->reps[0] : nullptr)) return bail(rc);
        Handle* h = (Handle*)hv;
        h->ens_member = r > 0;
        h->in_ensemble = true;
        e->reps.push_back(h);
    }
    e->frozen.assign((size_t)R, 0);
    e->uploads_seen.assign((size_t)R, 0);
    e->table.resize((size_t)R);
    if (hipMalloc((void**)&e->d_table, (size_t)R * sizeof(EnsRep)) != hipSuccess ||
        hipMalloc((void**)&e->d_ss_out, (size_t)R * sizeof(StepState)) != hipSuccess ||
        hipMalloc((void**)&e->d_n_out, (size_t)R * sizeof(int)) != hipSuccess ||
        hipEventCreate(&e->ev0) != hipSuccess || hipEventCreate(&e->ev1) != hipSuccess)
        return bail(fail("cetkmc_create_ensemble: device allocation failed"));
    {
        std::lock_guard<std::mutex> lk(g_ens_mu);
        g_ens[e->reps[0]] = e;
    }
    *handle = e->reps[0];
    return 0;
}

int cetkmc_ensemble_replica(void* handle, int r, void** replica)
{
    if (!handle || !replica) return fail("null argument");
    Ens* e = ens_of(handle);
    if (!e) return fail("not an ensemble handle (cetkmc_create_ensemble)");
    if (r < 0 || r >= e->R) return fail("replica index out of range");
    *replica = e->reps[(size_t)r];
    return 0;
}

int cetkmc_run_ensemble(void* handle, const cetkmc_ens_args* a, cetkmc_run_result* res, double* totals, double* dt)
{
    if (!handle || !a || !res) return fail("null argument");
    Ens* e = ens_of(handle);
    if (!e) return fail("not an ensemble handle (cetkmc_create_ensemble)");
    const int R = e->R, L = e->L;
    const int64_t n = a->n_steps;
    if (n < 0) return fail("n_steps < 0");
    if (a->rng_mode != 0 && a->rng_mode != 2) return fail("ensembles run rng_mode 0 (reference streams) or 2 (all counter based)");
    if (a->thermal_mode < 0 || a->thermal_mode > 2) return fail("thermal_mode must be 0 (none), 1 (diffusion) or 2 (laser source)");
    if (!a->defect_fraction) return fail("defect_fraction[R] required");
    // temperature updates of the call: the cadence is shared, so every replica's u-th update is the same global step
    const int64_t n_therm = a->thermal_mode ? updates_in(a->step0, n) : 0;
    const bool laser = a->thermal_mode == 2;
    if (e->ts.bc_on && a->thermal_mode) CHK(boundary_steps_ok("cetkmc_run_ensemble", e->ts.bc, a->step0, n));
    const bool beam = laser && e->ts.beam.on;       // the sources are rows of the ensemble's beam table: no plane sets
    if (beam) CHK(beam_args_ok("cetkmc_run_ensemble", e->ts.beam, a->q_planes, a->n_q, a->step0, n));
    if (laser && !beam) {       // everything about the plane sets is checked before anything is copied or launched
        if (a->n_q < n_therm) return fail("thermal_mode 2 needs one q plane per temperature update of the call in every plane set (n_q too small)");
        if (n_therm > 0 && !a->q_planes) return fail("thermal_mode 2: q_planes[n_sets][n_q][L*L] required (the call holds a temperature update)");
        if (!a->q_set && a->n_sets != R) return fail("thermal_mode 2: q_set NULL means plane set r for replica r, so n_sets must equal R");
        if (a->n_sets < 1) return fail("thermal_mode 2: n_sets must be >= 1");
        if (a->q_set)
            for (int r = 0; r < R; ++r)
                if (a->q_set[r] < 0 || a->q_set[r] >= a->n_sets) return fail("thermal_mode 2: q_set[" + std::to_string(r) + "] is outside [0, n_sets)");
    }
    bool any_defect = false;
    for (int r = 0; r < R; ++r) any_defect |= a->defect_fraction[r] > 0.0;
    const int64_t per_step = (int64_t)L * L + 2;         // at most L^2 deposition candidates + two orientation draws
    if (a->rng_mode == 0 && n > 0) {
        if (!a->u_pick || !a->u_np) return fail("rng_mode 0: u_pick[R][n] and u_np[R][np_stride] required");
        if (any_defect && !a->u_defect) return fail("rng_mode 0: u_defect[R][n] required when a defect_fraction is > 0");
        if (a->np_stride < n * per_step) return fail("rng_mode 0: np_stride must be >= n_steps * (L*L + 2)");
    }
    if (a->rng_mode == 2 && !a->seed) return fail("rng_mode 2: seed[R] required");
    for (Handle* h : e->reps)
        if (h->sweep_variant != 1 || !h->sweep_auto || h->thermal_variant != 1 || h->ifc_every_step || h->thermal_ahead)
            return fail("ensembles run the default kernel variants only (sweep_variant / thermal_variant / interface options untouched)");
    Handle* h0 = e->reps[0];
    for (Handle* h : e->reps)          // cetkmc_set_params on a replica must keep the shared fields shared
        if (!shared_params_equal(h0->p, h->p)) return fail(SHARED_PARAMS_MSG);
    for (Handle* h : e->reps) CHK(origin_room(h, n, "cetkmc_run_ensemble"));
    HIPCHK(hipSetDevice(h0->dev));
    HIPCHK(hipStreamSynchronize(h0->stream));
    hipStream_t st = h0->stream;
    const size_t nn = (size_t)std::max<int64_t>(n, 1);
    CHK(grow(&e->d_log_total, &e->cap_total, (size_t)R * nn));
    CHK(grow(&e->d_log_event, &e->cap_event, (size_t)R * nn));
    CHK(grow(&e->d_log_nev, &e->cap_nev, (size_t)R * nn));
    const bool streams = a->rng_mode == 0 && n > 0;
    const int64_t stride = streams ? a->np_stride : 0;
    if (streams) {
        CHK(grow(&e->d_u_pick, &e->cap_pick, (size_t)R * nn));
        CHK(grow(&e->d_u_np, &e->cap_np, (size_t)R * (size_t)stride));
        HIPCHK(hipMemcpyAsync(e->d_u_pick, a->u_pick, (size_t)R * n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(e->d_u_np, a->u_np, (size_t)R * stride * 8, hipMemcpyHostToDevice, st));
        if (any_defect) {
            CHK(grow(&e->d_u_defect, &e->cap_defect, (size_t)R * nn));
            HIPCHK(hipMemcpyAsync(e->d_u_defect, a->u_defect, (size_t)R * n * 8, hipMemcpyHostToDevice, st));
        }
    }
    const size_t L2 = (size_t)L * L;
    if (laser && !beam && n_therm > 0) {      // the first n_therm planes of every set, once per call: [n_sets][n_therm][L*L] on the device
        CHK(grow(&e->d_q, &e->cap_q, (size_t)a->n_sets * (size_t)n_therm * L2));
        HIPCHK(hipMemcpy2DAsync(e->d_q, (size_t)n_therm * L2 * 8, a->q_planes, (size_t)a->n_q * L2 * 8, (size_t)n_therm * L2 * 8,
                                (size_t)a->n_sets, hipMemcpyHostToDevice, st));
    }
    for (int r = 0; r < R; ++r)      // a new lattice uploaded into a terminated replica steps again
        if (e->reps[(size_t)r]->state_uploads != e->uploads_seen[(size_t)r]) {
            e->frozen[(size_t)r] = 0;
            e->uploads_seen[(size_t)r] = e->reps[(size_t)r]->state_uploads;
        }
    // per-replica table: both buffer pairs of each replica, relative to the pair current now (rel 0)
    for (int r = 0; r < R; ++r) {
        Handle* h = e->reps[(size_t)r];
        EnsRep& t = e->table[(size_t)r];
        t.kp = h->kp;
        for (int rel = 0; rel < 2; ++rel) {
            t.view[rel] = view_of(h, 0, h->cur ^ rel);
            t.sa[rel] = stream_args(h, t.view[rel]);
        }
        t.cfg = BatchCfg{};
        t.cfg.step0 = a->step0; t.cfg.defect_fraction = a->defect_fraction[r]; t.cfg.rng_mode = a->rng_mode; t.cfg.batch = 1;
        t.cfg.seed = a->rng_mode == 2 ? a->seed[r] : 0;
        t.cfg.np_cap = a->rng_mode == 2 ? INT64_MAX / 2 : stride;
        t.prev = h->slabs[0].prev; t.ss = h->d_ss; t.blocks = h->d_blocks; t.ktab = h->d_ktab; t.my_event = h->d_events_all;
        t.u_pick = streams ? e->d_u_pick + (size_t)r * n : nullptr;
        t.u_defect = (streams && any_defect) ? e->d_u_defect + (size_t)r * n : nullptr;
        t.u_np = streams ? e->d_u_np + (size_t)r * stride : nullptr;
        t.log_total = e->d_log_total + (size_t)r * nn; t.log_event = e->d_log_event + (size_t)r * nn; t.log_nev = e->d_log_nev + (size_t)r * nn;
        t.active = e->frozen[(size_t)r] ? 0 : 1;
        t.q = (laser && !beam && n_therm > 0) ? e->d_q + (size_t)(a->q_set ? a->q_set[r] : r) * (size_t)n_therm * L2 : nullptr;
    }
    HIPCHK(hipMemcpyAsync(e->d_table, e->table.data(), (size_t)R * sizeof(EnsRep), hipMemcpyHostToDevice, st));
    // the replica rides in y (in z, times the plane groups, for the temperature kernel)
    int ifc_blocks = 0;
    for (Handle* h : e->reps) ifc_blocks = std::max(ifc_blocks, h->ifc_blocks);
    const dim3 g_therm = thermal_grid(L, L, h0->therm_ni, R), g_table = table_grid(e->table[0].view[0], R);
    const dim3 g_ifc((unsigned)ifc_blocks, (unsigned)R), g_sweep((unsigned)L, (unsigned)R);
    // shared arguments: rate constants / thermal settings of replica 0 (equal in every replica but impurity_c, nu_dep)
    const StreamArgs sa0{};
    const KParams kp0 = h0->kp;
    const double K0 = host_k_eff(h0->p, 0, 0);
    const SlabView v0{};
    const int latent = laser && a->use_latent ? 1 : 0;
    // every update of the call is made alike (one n, one scheme, one boundary for every replica) but for the update ordinal
    const UpdatePlan P0 = plan_update(e->ts, h0->p, a->thermal_dt, 0);
    const ThermalCfg tc0 = thermal_cfg(h0, P0.dt_s, laser ? 1 : 0, latent, 1), tc_sub = thermal_cfg(h0, P0.dt_s, laser ? 1 : 0, 0, 0);
    const double* coef = nullptr;       // the coefficient table of replica 0 serves every replica
    if (P0.implicit && n_therm > 0) CHK(plan_coeffs(h0, e->ts, P0, e->ti, &coef));
    const ImpCfg ic0 = imp_cfg(h0->p, P0, coef, laser ? 1 : 0, latent, 1), ic_sub = imp_cfg(h0->p, P0, coef, laser ? 1 : 0, 0, 0);
    const BatchCfg cfg0{};
    const dim3 g_flags((unsigned)std::min<int64_t>(((int64_t)(L + 4) * L + 255) / 256, 64), (unsigned)R);
    EnsSel sel{e->d_table, 0, (int)g_therm.z / R};
    auto table_and_interface = [&]() {
        launch(k_rate_table<EnsSel>, g_table, dim3(256), 0, st, nullptr, nullptr, kp0, v0, K0, nullptr, sel);
        launch(k_interface<EnsSel>, g_ifc, dim3(256), 0, st, nullptr, nullptr, kp0, v0, nullptr, nullptr, sel);
    };
    HIPCHK(hipEventRecord(e->ev0, st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_batch_reset<EnsSel>), dim3((unsigned)R), dim3(1), 0, st, (StepState*)nullptr, sel);
    // rate table + interface sums of the fields as they stand (an upload, a defect refresh or a per-replica call may
    // have left them stale; recomputing fresh ones gives the same values) -- unless the first step's update does it
    if (!(a->thermal_mode && n > 0 && a->step0 % 20 == 0)) table_and_interface();
    int flips = 0;
    // the kernel that wrote the other buffer pair has also brought prev_state level with state on the flagged rows: the first step
    // of a latent update drops the flags (live replicas); from here on the other pair is the current one
    auto flip = [&](bool first) {
        if (first && latent) hipLaunchKernelGGL(k_ens_clear_row_flags, g_flags, dim3(256), 0, st, (const EnsRep*)e->d_table);
        sel.rel ^= 1;
        ++flips;
    };
    for (int64_t s = 0; s < n; ++s) {
        const int64_t g = a->step0 + s;
        if (a->thermal_mode && g % 20 == 0) {          // kmc_simulation.py:248-250, shared cadence
            const UpdatePlan P = plan_update(e->ts, h0->p, a->thermal_dt, g / 20, laser);
            for (int q = 0; q < P.n; ++q) {        // steps 2..n: no scrub, no latent term, same plane
                // an implicit step (thermal_imp.hpp): three launches, the flip behind the row pass (the line passes work in place)
                if (P.implicit) launch_imp_step(st, L, R, P, q == 0 ? ic0 : ic_sub, v0, nullptr, nullptr, nullptr, nullptr, nullptr, [&] { flip(q == 0); }, sel);
                else {
                    launch(k_thermal_march<EnsSel>, g_therm, dim3(256), 0, st, nullptr, nullptr, v0, nullptr, nullptr, nullptr, nullptr, q == 0 ? tc0 : tc_sub, nullptr, sel);
                    flip(q == 0);
                }
            }
            count_update(e->ti, P, (P.implicit ? 3 : 1) * (int64_t)P.n);
            sel.q_off += laser ? (int64_t)L2 : 0;
            if (e->ts.remelt_on)       // behind the update and its prev_state := state, in front of the table and the interface kernel
                launch_melt_pass(st, e->table[0].view[0], R, v0, nullptr, MeltState{}, e->d_melt_tab, e->ts.remelt_threshold, nullptr, sel);
            table_and_interface();
        }
        launch(k_sweep_plane<true, false, EnsSel>, g_sweep, dim3(1024), plane_shmem(L), st, nullptr, nullptr, sa0, nullptr, nullptr, sel);
        launch(k_select_apply<true, EnsSel>, dim3((unsigned)R), dim3(256), 0, st, nullptr, nullptr, kp0, nullptr, 1, L, h0->PB, nullptr,
               nullptr, cfg0, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, (long long)s, sel);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->ev1, st));
    hipLaunchKernelGGL(k_ens_collect, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, st, (const EnsRep*)e->d_table, R, e->d_ss_out, e->d_n_out);
    HIPCHK(hipGetLastError());
    const bool melt_read = e->ts.remelt_on && e->d_melt_tab;       // only a call that may have run a pass gathers the counters
    std::vector<unsigned long long> melt_cnt(melt_read ? (size_t)R * 4 : 0);       // the remelt counters travel with the results
    if (melt_read) {
        launch(k_melt_collect, dim3((unsigned)((4 * R + 255) / 256)), dim3(256), 0, st, nullptr, nullptr, e->d_melt_tab, R, e->d_melt_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(melt_cnt.data(), e->d_melt_out, melt_cnt.size() * 8, hipMemcpyDeviceToHost, st));
    }
    std::vector<StepState> ss((size_t)R);
    std::vector<int> list_len((size_t)R);
    std::vector<uint8_t> t_active((size_t)R);           // stepped by this call (not frozen when it began)
    for (int r = 0; r < R; ++r) t_active[(size_t)r] = e->frozen[(size_t)r] ? 0 : 1;
    std::vector<double> tot(n > 0 ? (size_t)R * n : 0);
    HIPCHK(hipMemcpyAsync(ss.data(), e->d_ss_out, (size_t)R * sizeof(StepState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(list_len.data(), e->d_n_out, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, st));
    if (n > 0) HIPCHK(hipMemcpy2DAsync(tot.data(), (size_t)n * 8, e->d_log_total, nn * 8, (size_t)n * 8, (size_t)R, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->ev0, e->ev1));
    for (int r = 0; r < R; ++r)       // (cannot happen: np_stride covers the worst case) -- checked before any replica changes
        if (ss[(size_t)r].status == 2) return fail("ensemble replica ran out of its NumPy stream (np_stride too small)");
    for (int r = 0; r < R; ++r) {
        Handle* h = e->reps[(size_t)r];
        const StepState& q = ss[(size_t)r];
        if (melt_read) melt_info_from(h, melt_cnt.data() + 4 * (size_t)r);
        h->cur ^= flips & 1;
        invalidate(h, Cause::ensemble_stepped);      // recompute on demand
        grow_ifc_grid(h, list_len[(size_t)r]);
        h->cnt.steps += q.cur;
        if (q.status == 1) e->frozen[(size_t)r] = 1;
        cetkmc_run_result& o = res[r];
        o = cetkmc_run_result{};
        o.steps_done = q.cur; o.status = q.status; o.np_used = a->rng_mode == 0 ? q.np_pos : 0;
        if (laser && t_active[(size_t)r]) {
            // planes consumed, as on a single handle: the updates of the executed steps and of the step the replica stopped
            // in (its update precedes the selection that noticed the stop); later updates were pass-throughs
            o.q_used = q.status == 0 ? n_therm : updates_in(a->step0, std::min(q.cur + 1, n));
        }
        o.nucleation_count = q.nuc_count; o.min_margin = q.min_margin; o.wall_ms = ms; o.full_sweeps = q.cur;
        const int64_t done = q.cur;
        if (totals) {
            double* row = totals + (size_t)r * (n + 1);
            for (int64_t s = 0; s < done; ++s) row[s] = tot[(size_t)r * n + s];
            if (q.status == 1 && done <= n) row[done] = q.total;
        }
        if (dt && a->rng_mode == 2)
            for (int64_t s = 0; s < done; ++s) dt[(size_t)r * n + s] = superstep_dt_event(a->seed[r], a->step0 + s, tot[(size_t)r * n + s]);
    }
    if (e->d_origin_block && h0->origin_on && n > 0) {
        // every replica's executed steps join its origin map: its log from the replica table, its clock and step count from a
        // run table pushed once, one launch whatever R
        e->origin_runs.resize((size_t)R);
        for (int r = 0; r < R; ++r) {
            Handle* h = e->reps[(size_t)r];
            e->origin_runs[(size_t)r] = OriginRun{(long long)h->origin_seq, (long long)ss[(size_t)r].cur};
            h->origin_seq += ss[(size_t)r].cur;
        }
        HIPCHK(hipMemcpyAsync(e->d_origin_runs, e->origin_runs.data(), (size_t)R * sizeof(OriginRun), hipMemcpyHostToDevice, st));
        const EnsSel osel{e->d_table, 0, 0, 0, nullptr};
        launch(k_origin_absorb<EnsSel>, dim3((unsigned)((n + 255) / 256), (unsigned)R), dim3(256), 0, st, nullptr, nullptr, nullptr, 0LL, 1LL, 0LL, L,
               OriginMap{}, (const OriginMap*)e->d_origin_maps, (const OriginRun*)e->d_origin_runs, osel);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// ---- batched analysis of every replica (metrics rows of run_kmc_ensemble): launches independent of R ----------------------
static int ens_push_views(Ens* e)
{
    for (int r = 0; r < e->R; ++r) {
        Handle* h = e->reps[(size_t)r];
        e->table[(size_t)r].view[0] = view_of(h, 0, h->cur);
        e->table[(size_t)r].view[1] = view_of(h, 0, h->cur ^ 1);
        e->table[(size_t)r].ss = h->d_ss;      // k_ens_collect reads it: an analysis may precede the ensemble's first run
        e->table[(size_t)r].kp = h->kp;        // (k_front_stats: T_melt of the replica's own parameters)
    }
    HIPCHK(hipMemcpyAsync(e->d_table, e->table.data(), (size_t)e->R * sizeof(EnsRep), hipMemcpyHostToDevice, e->reps[0]->stream));
    return 0;
}

int cetkmc_ensemble_analyze(void* handle, cetkmc_ens_analysis* a)
{
    if (!handle || !a) return fail("null argument");
    Ens* e = ens_of(handle);
    if (!e) return fail("not an ensemble handle (cetkmc_create_ensemble)");
    if (!a->n_clusters || !a->species_counts || !a->nucleation_count || (a->species >= 0 && !a->n_gathered)) return fail("null output array");
    const int R = e->R, L = e->L;
    const int64_t n = (int64_t)L * L * L;
    Handle* h0 = e->reps[0];
    hipStream_t st = h0->stream;
    HIPCHK(hipSetDevice(h0->dev));
    if (!e->d_cc_parent) {
        const size_t m = (size_t)R * n;
        HIPCHK(hipMalloc((void**)&e->d_cc_parent, m * sizeof(int)));
        HIPCHK(hipMalloc((void**)&e->d_cc_cid, m * sizeof(int)));
        HIPCHK(hipMalloc((void**)&e->d_cc_roots, m * sizeof(int)));
        HIPCHK(hipMalloc((void**)&e->d_cc_labels, m * sizeof(int)));
        HIPCHK(hipMalloc((void**)&e->d_cc_n, (size_t)R * sizeof(int)));
        HIPCHK(hipMalloc((void**)&e->d_cc_offs, (size_t)(R + 1) * sizeof(long long)));
        HIPCHK(hipMalloc((void**)&e->d_counts, (size_t)R * 6 * sizeof(unsigned long long)));
        HIPCHK(hipMalloc((void**)&e->d_g_n, (size_t)R * sizeof(unsigned long long)));
    }
    if (a->species >= 0 && !e->d_g_idx) {         // worst case: every voxel of a replica in the species
        HIPCHK(hipMalloc((void**)&e->d_g_idx, (size_t)R * n * sizeof(long long)));
        HIPCHK(hipMalloc((void**)&e->d_g_T, (size_t)R * n * sizeof(double)));
    }
    CHK(ens_push_views(e));
    EnsSel sel{e->d_table, 0, 0, n, e->d_cc_offs};
    const SlabView v0{};
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
    const dim3 g(grid, (unsigned)R), gs(std::min(grid, 256u), (unsigned)R);
    HIPCHK(hipMemsetAsync(e->d_cc_n, 0, (size_t)R * sizeof(int), st));
    HIPCHK(hipMemsetAsync(e->d_counts, 0, (size_t)R * 6 * sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(e->d_g_n, 0, (size_t)R * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cc_init<EnsSel>), g, dim3(256), 0, st, v0, e->d_cc_parent, sel);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cc_hook<EnsSel>), g, dim3(256), 0, st, v0, e->d_cc_parent, a->threshold, sel);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cc_compress<EnsSel>), g, dim3(256), 0, st, n, e->d_cc_parent, e->d_cc_roots, e->d_cc_n, sel);
    hipLaunchKernelGGL(k_ens_cc_rank, dim3((unsigned)R), dim3(1024), 0, st, (const int*)e->d_cc_parent, e->d_cc_cid, e->d_cc_roots,
                       e->d_cc_n, n);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_species_counts<EnsSel>), gs, dim3(256), 0, st, v0, e->d_counts, sel);
    if (a->species >= 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gather_species<EnsSel>), gs, dim3(256), 0, st, v0, (int)a->species, e->d_g_idx, e->d_g_T,
                           (unsigned long long)n, e->d_g_n, sel);
    hipLaunchKernelGGL(k_ens_collect, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, st, (const EnsRep*)e->d_table, R, e->d_ss_out, e->d_n_out);
    HIPCHK(hipGetLastError());
    std::vector<int> nr((size_t)R);
    std::vector<unsigned long long> cnt((size_t)R * 6), gn((size_t)R);
    std::vector<StepState> ss((size_t)R);
    HIPCHK(hipMemcpyAsync(nr.data(), e->d_cc_n, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cnt.data(), e->d_counts, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(gn.data(), e->d_g_n, gn.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(ss.data(), e->d_ss_out, (size_t)R * sizeof(StepState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // per-cluster size / bounding box: the replicas' clusters concatenated (entry offs[r] + id - 1)
    std::vector<long long> offs((size_t)R + 1, 0);
    for (int r = 0; r < R; ++r) offs[(size_t)r + 1] = offs[(size_t)r] + nr[(size_t)r];
    const int64_t total = offs[(size_t)R];
    CHK(grow(&e->d_cc_stats, &e->cap_cc_stats, (size_t)std::max<int64_t>(total, 1) * 8));
    HIPCHK(hipMemcpyAsync(e->d_cc_offs, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    if (total > 0) hipLaunchKernelGGL(k_cc_stats_init, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (int)total, e->d_cc_stats);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cc_stats<EnsSel>), g, dim3(256), 0, st, v0, (const int*)e->d_cc_parent, (const int*)e->d_cc_cid,
                       e->d_cc_labels, e->d_cc_stats, sel);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    e->an_clusters.assign((size_t)R, 0);
    e->an_gathered.assign((size_t)R, 0);
    e->an_species = a->species;
    for (int r = 0; r < R; ++r) {
        e->an_clusters[(size_t)r] = a->n_clusters[r] = nr[(size_t)r];
        for (int c = 0; c < 6; ++c) a->species_counts[6 * r + c] = (int64_t)cnt[(size_t)6 * r + c];
        a->nucleation_count[r] = ss[(size_t)r].nuc_count;
        if (a->species >= 0) e->an_gathered[(size_t)r] = a->n_gathered[r] = (int64_t)gn[(size_t)r];
    }
    return 0;
}

int cetkmc_ensemble_analysis_data(void* handle, int32_t* first_voxel, int64_t* size, int32_t* bbox, int32_t* labels, int64_t* lin_idx,
                                  double* T_vals)
{
    if (!handle) return fail("null argument");
    Ens* e = ens_of(handle);
    if (!e) return fail("not an ensemble handle (cetkmc_create_ensemble)");
    if (e->an_clusters.empty()) return fail("cetkmc_ensemble_analysis_data needs a preceding cetkmc_ensemble_analyze");
    const int R = e->R, L = e->L;
    const int64_t n = (int64_t)L * L * L;
    Handle* h0 = e->reps[0];
    hipStream_t st = h0->stream;
    HIPCHK(hipSetDevice(h0->dev));
    int64_t total = 0, maxc = 0, maxg = 0;
    for (int r = 0; r < R; ++r) { total += e->an_clusters[(size_t)r]; maxc = std::max(maxc, e->an_clusters[(size_t)r]); maxg = std::max(maxg, e->an_gathered[(size_t)r]); }
    std::vector<int> roots, stats((size_t)std::max<int64_t>(total, 1) * 8);
    std::vector<long long> gi;
    std::vector<double> gT;
    if (maxc > 0 && (first_voxel || size || bbox)) {
        roots.resize((size_t)R * maxc);
        HIPCHK(hipMemcpy2DAsync(roots.data(), (size_t)maxc * 4, e->d_cc_roots, (size_t)n * 4, (size_t)maxc * 4, (size_t)R, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(stats.data(), e->d_cc_stats, (size_t)total * 8 * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    if (labels) HIPCHK(hipMemcpyAsync(labels, e->d_cc_labels, (size_t)R * n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (maxg > 0 && e->an_species >= 0 && (lin_idx || T_vals)) {
        gi.resize((size_t)R * maxg); gT.resize((size_t)R * maxg);
        HIPCHK(hipMemcpy2DAsync(gi.data(), (size_t)maxg * 8, e->d_g_idx, (size_t)n * 8, (size_t)maxg * 8, (size_t)R, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpy2DAsync(gT.data(), (size_t)maxg * 8, e->d_g_T, (size_t)n * 8, (size_t)maxg * 8, (size_t)R, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    int64_t q = 0, p = 0;
    for (int r = 0; r < R; ++r) {
        for (int64_t c = 0; c < e->an_clusters[(size_t)r] && !roots.empty(); ++c, ++q) {
            const int v = roots[(size_t)r * maxc + c];
            if (first_voxel) { first_voxel[3 * q] = v / (L * L); first_voxel[3 * q + 1] = (v / L) % L; first_voxel[3 * q + 2] = v % L; }
            if (size) size[q] = stats[(size_t)8 * q];
            if (bbox) for (int k = 0; k < 6; ++k) bbox[6 * q + k] = stats[(size_t)8 * q + 1 + k];
        }
        for (int64_t c = 0; c < e->an_gathered[(size_t)r] && !gi.empty(); ++c, ++p) {
            if (lin_idx) lin_idx[p] = gi[(size_t)r * maxg + c];
            if (T_vals) T_vals[p] = gT[(size_t)r * maxg + c];
        }
    }
    return 0;
}

int cetkmc_ensemble_cluster_import(void* handle, const int32_t* labels, int64_t* n_clusters)
{
    if (!handle || !labels || !n_clusters) return fail("null argument");
    Ens* e = ens_of(handle);
    if (!e) return fail("not an ensemble handle (cetkmc_create_ensemble)");
    if (e->an_clusters.empty()) return fail("cetkmc_ensemble_cluster_import needs a preceding cetkmc_ensemble_analyze");
    const int R = e->R, L = e->L;
    const int64_t n = (int64_t)L * L * L;
    // every replica is checked before anything is uploaded: one bad replica leaves the previous analysis as it is
    std::vector<int> roots, stats, r1, s1;
    std::vector<long long> offs((size_t)R + 1, 0);
    for (int r = 0; r < R; ++r) {
        CHK(cc_import_scan("cetkmc_ensemble_cluster_import", labels + (int64_t)r * n, L, r, r1, s1));
        roots.insert(roots.end(), r1.begin(), r1.end());
        stats.insert(stats.end(), s1.begin(), s1.end());
        offs[(size_t)r + 1] = offs[(size_t)r] + (long long)r1.size();
    }
    const int64_t total = offs[(size_t)R];
    Handle* h0 = e->reps[0];
    hipStream_t st = h0->stream;
    HIPCHK(hipSetDevice(h0->dev));
    HIPCHK(hipStreamSynchronize(st));
    CHK(grow(&e->d_cc_stats, &e->cap_cc_stats, (size_t)std::max<int64_t>(total, 1) * 8));
    HIPCHK(hipMemcpyAsync(e->d_cc_offs, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    for (int r = 0; r < R; ++r) {        // a replica's roots at r * L^3, as k_cc_compress leaves them
        const long long a = offs[(size_t)r], k = offs[(size_t)r + 1] - a;
        if (k > 0) HIPCHK(hipMemcpyAsync(e->d_cc_roots + (int64_t)r * n, roots.data() + a, (size_t)k * sizeof(int), hipMemcpyHostToDevice, st));
    }
    if (total > 0) HIPCHK(hipMemcpyAsync(e->d_cc_stats, stats.data(), (size_t)total * 8 * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(e->d_cc_labels, labels, (size_t)R * n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    h0->cnt.bytes_h2d += (int64_t)(((size_t)R * n + (size_t)total * 9) * sizeof(int) + offs.size() * sizeof(long long));
    for (int r = 0; r < R; ++r) e->an_clusters[(size_t)r] = n_clusters[r] = offs[(size_t)r + 1] - offs[(size_t)r];
    return 0;
}

int cetkmc_ensemble_set_defects_sparse(void* handle, const int64_t* counts, const int64_t* lin_idx)
{
    if (!handle || !counts) return fail("null argument");
    Ens* e = ens_of(handle);
    if (!e) return fail("not an ensemble handle (cetkmc_create_ensemble)");
    const int R = e->R, L = e->L;
    Handle* h0 = e->reps[0];
    hipStream_t st = h0->stream;
    HIPCHK(hipSetDevice(h0->dev));
    std::vector<long long> offs((size_t)2 * R);
    int64_t total = 0, maxn = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t c = counts[r];
        offs[(size_t)2 * r] = c < 0 ? -1 : total;
        offs[(size_t)2 * r + 1] = c < 0 ? -1 : total + c;
        if (c > 0) { total += c; maxn = std::max(maxn, c); }
    }
    if (total > 0 && !lin_idx) return fail("null argument");
    for (int64_t q = 0; q < total; ++q)
        if (lin_idx[q] < 0 || lin_idx[q] >= (int64_t)L * L * L) return fail("linear index out of range");
    if (!e->d_sc_offs) HIPCHK(hipMalloc((void**)&e->d_sc_offs, (size_t)2 * R * sizeof(long long)));
    CHK(grow(&e->d_sc_idx, &e->cap_sc_idx, (size_t)std::max<int64_t>(total, 1)));
    CHK(ens_push_views(e));
    HIPCHK(hipMemcpyAsync(e->d_sc_offs, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    if (total > 0) HIPCHK(hipMemcpyAsync(e->d_sc_idx, lin_idx, (size_t)total * sizeof(long long), hipMemcpyHostToDevice, st));
    EnsSel sel{e->d_table, 0, 0, 0, e->d_sc_offs};
    hipLaunchKernelGGL(k_ens_clear_defects, dim3(256, (unsigned)R), dim3(256), 0, st, (const EnsRep*)e->d_table, (const long long*)e->d_sc_offs);
    if (maxn > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_scatter_defects<EnsSel>), dim3((unsigned)std::min<int64_t>((maxn + 255) / 256, 4096), (unsigned)R),
                           dim3(256), 0, st, SlabView{}, (const long long*)e->d_sc_idx, 0LL, sel);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    for (int r = 0; r < R; ++r)
        if (counts[r] >= 0) invalidate(e->reps[(size_t)r], Cause::set_defects);
    return 0;
}

// ---- diagnostics: what a pass runs over ---------------------------------------------------------
// Every diagnostic below is ONE body, entered twice: cetkmc_x for one lattice, cetkmc_ensemble_x for every replica of an
// ensemble.  lattices() turns (the entry point's name, its handle, which of the two it is, what the pass needs) into a
// Lattices or the refusal; the body issues its launches through Lattices::run, which appends the ensemble's selector to the
// kernel's arguments or nothing at all.  A new diagnostic is one more such body and two entry points.
extern "C++" {
enum EnsUse { ENS_VIEWS, ENS_LABELS, ENS_GRAINS };      // what the kernel takes per replica: its view; + its labels; + its grains
struct Lattices {
    Handle* h0 = nullptr;            // the handle the pass is issued on: its stream, counters and scratch buffers
    Ens* e = nullptr;                // null: one lattice
    std::vector<Handle*> hs;         // the R lattices
    hipStream_t stream = nullptr;
    int L = 0, R = 1;
    SlabView view{};                 // the lattice's view (an ensemble's kernels take theirs from the replica table)
    // the clustering in force (cetkmc_cluster / _cluster_import, cetkmc_ensemble_analyze / _cluster_import); grains < 0: none
    const int *labels = nullptr, *roots = nullptr, *stats = nullptr;
    int64_t grains = -1, max_grains = 0;      // of all lattices together, of the lattice that has most
    int n = 0;                                // the kernels' grain count (an ensemble's take theirs from the offsets)
    // f(ens...) with no argument or with the ensemble's selector: launch(k_x<decltype(ens)...>, ..., ens...)
    template <class F> void run(EnsUse use, F&& f) const
    {
        if (e) f(EnsSel{e->d_table, 0, 0, use == ENS_VIEWS ? 0 : (int64_t)L * L * L, use == ENS_GRAINS ? e->d_cc_offs : nullptr});
        else f();
    }
    // blocks of 256 threads over the grains of a lattice (grid-stride kernels), times the lattices
    dim3 grain_grid(int64_t blocks) const { return dim3((unsigned)std::min<int64_t>(blocks, 4096), (unsigned)R); }
};
}
// needs: ONE_LATTICE refuses an ensemble's own handle (a replica is a lattice), OWNER anything but a handle that keeps its own
// maps; CLUSTERS a clustering; SOLID / ORIGIN name the map family, MAP asks for its maps to be on; VIEWS: the ensemble's
// kernels read the replicas' views
enum : unsigned { ONE_LATTICE = 1, OWNER = 2, CLUSTERS = 4, SOLID = 8, ORIGIN = 16, MAP = 32, VIEWS = 64 };
static std::string no_clusters(const char* fn, bool ens) { return std::string(fn) + (ens ? " needs a preceding cetkmc_ensemble_analyze" : " needs a preceding cetkmc_cluster"); }
static std::string no_map(const char* fn, bool ens, unsigned needs)
{
    const std::string fam = needs & SOLID ? "solid" : "origin";
    return std::string(fn) + (ens ? " needs the maps (cetkmc_ensemble_" : " needs a map (cetkmc_") + fam + "_begin)";
}
static int lattices(const char* fn, void* handle, bool ens, unsigned needs, Lattices* out)
{
    const std::string f(fn);
    Lattices& A = *out;
    if (!handle) return fail(!ens && (needs & OWNER) ? "null handle" : "null argument");
    if (ens) {
        Ens* e = A.e = ens_of(handle);
        if (!e) return fail("not an ensemble handle (cetkmc_create_ensemble)");
        A.h0 = e->reps[0]; A.hs = e->reps; A.R = e->R;
        if ((needs & MAP) && !((needs & SOLID ? e->d_solid_block && A.h0->solid_on : e->d_origin_block && A.h0->origin_on)))
            return fail(no_map(fn, true, needs));
        if (!e->an_clusters.empty()) {
            A.labels = e->d_cc_labels; A.roots = e->d_cc_roots; A.stats = e->d_cc_stats; A.grains = 0;
            for (int64_t c : e->an_clusters) { A.grains += c; A.max_grains = std::max(A.max_grains, c); }
        }
    } else {
        Handle* h = A.h0 = (Handle*)handle;
        if ((needs & ONE_LATTICE) && ens_of(handle)) return fail(f + " takes one lattice: an ensemble handle goes to cetkmc_ensemble_" + (fn + 7));
        if ((needs & OWNER) && h->in_ensemble)
            return fail(f + " takes a single-lattice handle: an ensemble's maps are kept by cetkmc_ensemble_" + (needs & SOLID ? "solid_*" : "origin_*"));
        if (h->slabs.size() != 1 || h->nranks != 1) return fail(f + " needs the whole lattice in one slab");
        if ((needs & MAP) && !(needs & SOLID ? h->solid_on : h->origin_on)) return fail(no_map(fn, false, needs));
        A.hs = {h}; A.view = view_of(h, 0);
        if (h->cc_n_clusters >= 0) {
            A.labels = h->d_cc_labels; A.roots = h->d_cc_roots; A.stats = h->d_cc_stats;
            A.grains = A.max_grains = h->cc_n_clusters; A.n = (int)h->cc_n_clusters;
        }
    }
    if ((needs & CLUSTERS) && A.grains < 0) return fail(no_clusters(fn, ens));
    A.stream = A.h0->stream; A.L = A.h0->L;
    HIPCHK(hipSetDevice(A.h0->dev));
    if (A.e && (needs & VIEWS)) CHK(ens_push_views(A.e));
    return 0;
}

// n_lay + n_gr records of NW words W for a pass: initialised on the stream (init: the k_*_rec_init kernel; null: zeroes),
// filled (go = the launches, or its error) and copied out, n_lay records to `layers` and the first n_copy of the others to `grains`
extern "C++" template <class W, class Go>
static int fill_records(Handle* h, hipStream_t st, const char* what, int NW, void (*init)(W*, int64_t), int64_t n_lay, int64_t n_gr, int64_t n_copy,
                        void* layers, void* grains, Go&& go)
{
    DevTmp<W> d_rec;
    const int64_t words = (n_lay + n_gr) * NW, rec_bytes = NW * (int64_t)sizeof(W);
    if (d_rec.alloc((size_t)words) != hipSuccess) {
        (void)hipGetLastError();
        return fail(std::string(what) + ": no device memory for " + std::to_string(n_lay + n_gr) + " records of " + std::to_string(rec_bytes) + " bytes");
    }
    if (init) launch(init, dim3((unsigned)std::min<int64_t>((words + 255) / 256, 4096)), dim3(256), 0, st, nullptr, nullptr, d_rec.p, words);
    else HIPCHK(hipMemsetAsync(d_rec.p, 0, (size_t)(words * (int64_t)sizeof(W)), st));
    CHK(go(d_rec.p, d_rec.p + n_lay * NW));
    HIPCHK(hipGetLastError());
    if (n_lay > 0) HIPCHK(hipMemcpyAsync(layers, d_rec.p, (size_t)(n_lay * rec_bytes), hipMemcpyDeviceToHost, st));
    if (n_copy > 0) HIPCHK(hipMemcpyAsync(grains, d_rec.p + n_lay * NW, (size_t)(n_copy * rec_bytes), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    h->cnt.bytes_d2h += (n_lay + std::max<int64_t>(n_copy, 0)) * rec_bytes;
    return 0;
}

// ---- solidification-front diagnostics (front.hpp) ----------------------------------------------
static dim3 front_grid(int L, int R)
{
    return dim3((unsigned)(((L + FRONT_TJ - 1) / FRONT_TJ) * ((L + FRONT_TK - 1) / FRONT_TK)), (unsigned)((L + FRONT_NI - 1) / FRONT_NI),
                (unsigned)R);
}

static int front_stats(const char* fn, void* handle, bool ens, double inv_dx, struct cetkmc_front_stats* out)
{
    if (!handle || !out) return fail("null argument");
    Lattices A;
    CHK(lattices(fn, handle, ens, VIEWS, &A));
    Handle* h = A.h0;
    const dim3 g = front_grid(A.L, A.R);
    const int nb = (int)(g.x * g.y);
    CHK(grow(&h->d_front_part, &h->cap_front_part, (size_t)A.R * nb));      // [R][blocks of a lattice] partials, [R] results
    CHK(grow(&h->d_front_out, &h->cap_front_out, (size_t)A.R));
    A.run(ENS_VIEWS, [&](auto... sel) {      // (a replica's kernel takes T_melt from its own parameters)
        launch(k_front_stats<decltype(sel)...>, g, dim3(256), 0, A.stream, nullptr, nullptr, A.view, h->kp.T_melt, inv_dx, h->d_front_part, sel...);
    });
    launch(k_front_fold, dim3((unsigned)A.R), dim3(256), 0, A.stream, nullptr, nullptr, h->d_front_part, nb, A.L, h->d_front_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_front_out, (size_t)A.R * sizeof(FrontStats), hipMemcpyDeviceToHost, A.stream));
    HIPCHK(hipStreamSynchronize(A.stream));
    h->cnt.bytes_d2h += (int64_t)A.R * (int64_t)sizeof(FrontStats);
    return 0;
}
int cetkmc_front_stats(void* handle, double inv_dx, struct cetkmc_front_stats* out) { return front_stats("cetkmc_front_stats", handle, false, inv_dx, out); }
int cetkmc_ensemble_front_stats(void* handle, double inv_dx, struct cetkmc_front_stats* out)
{
    return front_stats("cetkmc_ensemble_front_stats", handle, true, inv_dx, out);
}

// ---- layer-resolved grain structure (layer.hpp) ------------------------------------------------
static dim3 layer_grid(int L, int R)
{
    return dim3((unsigned)(((L + LAYER_TJ - 1) / LAYER_TJ) * ((L + LAYER_TK - 1) / LAYER_TK)), (unsigned)((L + LAYER_NI - 1) / LAYER_NI),
                (unsigned)R);
}

static int layer_profile(const char* fn, void* handle, bool ens, double ar_threshold, struct cetkmc_layer_rec* out)
{
    if (!handle || !out) return fail("null argument");
    Lattices A;
    CHK(lattices(fn, handle, ens, ONE_LATTICE | CLUSTERS | VIEWS, &A));
    Handle* h = A.h0;
    const int L = A.L, R = A.R;
    const dim3 g = layer_grid(L, R);
    CHK(grow(&h->d_layer_eq, &h->cap_layer_eq, (size_t)(A.grains + R)));          // a lattice has one more byte than grains
    CHK(grow(&h->d_layer_part, &h->cap_layer_part, (size_t)R * L * g.x));         // [R][L][tiles] partials, [R][L] records
    CHK(grow(&h->d_layer_out, &h->cap_layer_out, (size_t)R * L));
    A.run(ENS_GRAINS, [&](auto... sel) {
        launch(k_layer_class<decltype(sel)...>, A.grain_grid(A.max_grains / 256 + 1), dim3(256), 0, A.stream, nullptr, nullptr, A.stats, A.n, ar_threshold,
               h->d_layer_eq, sel...);
        launch(k_layer_profile<decltype(sel)...>, g, dim3(256), 0, A.stream, nullptr, nullptr, A.view, A.labels, A.roots, h->d_layer_eq, h->d_layer_part,
               sel...);
    });
    launch(k_layer_fold, dim3((unsigned)L, (unsigned)R), dim3(64), 0, A.stream, nullptr, nullptr, h->d_layer_part, (int)g.x, h->d_layer_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, h->d_layer_out, (size_t)R * L * sizeof(LayerRec), hipMemcpyDeviceToHost, A.stream));
    HIPCHK(hipStreamSynchronize(A.stream));
    h->cnt.bytes_d2h += (int64_t)R * L * (int64_t)sizeof(LayerRec);
    return 0;
}
int cetkmc_layer_profile(void* handle, double ar_threshold, struct cetkmc_layer_rec* out)
{
    return layer_profile("cetkmc_layer_profile", handle, false, ar_threshold, out);
}
int cetkmc_ensemble_layer_profile(void* handle, double ar_threshold, struct cetkmc_layer_rec* out)
{
    return layer_profile("cetkmc_ensemble_layer_profile", handle, true, ar_threshold, out);
}

// ---- grain-boundary misorientation and pole histograms (texture.hpp) ---------------------------
// the caller's arguments checked and turned into the kernel's: everything a refusal needs is known here, on the host
static int texture_args(const char* fn, const struct cetkmc_texture_args* a, TexArgs* A)
{
    const std::string f(fn);
    if (a->n_bins < 1 || a->n_bins > TEX_MAX_BINS) return fail(f + ": n_bins " + std::to_string(a->n_bins) + " outside 1.." + std::to_string(TEX_MAX_BINS));
    const double* src[2] = {a->gb_edges, a->pole_edges};
    const char* const name[2] = {"gb_edges", "pole_edges"};
    A->n_bins = a->n_bins; A->pad = 0;
    for (int w = 0; w < 2; ++w) {
        if (a->n_bins > 1 && !src[w]) return fail(f + ": " + name[w] + " is NULL with n_bins > 1");
        for (int q = 0; q < TEX_NE; ++q) {
            if (q >= a->n_bins - 1) { A->edges[w][q] = -HUGE_VAL; continue; }
            const double e = src[w][q];
            if (!std::isfinite(e)) return fail(f + ": " + name[w] + "[" + std::to_string(q) + "] is not finite");
            if (q > 0 && !(e < src[w][q - 1])) return fail(f + ": " + name[w] + "[" + std::to_string(q) + "] is not below its predecessor (strictly decreasing edges)");
            A->edges[w][q] = e;
        }
    }
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(a->axis[c])) return fail(f + ": axis[" + std::to_string(c) + "] is not finite");
        A->axis[c] = a->axis[c];
    }
    return 0;
}
static dim3 texture_grid(int L, int R)
{
    return dim3((unsigned)(((L + TEX_TJ - 1) / TEX_TJ) * ((L + TEX_TK - 1) / TEX_TK)), (unsigned)((L + TEX_NI - 1) / TEX_NI), (unsigned)R);
}
// zero the rows on the stream, count into them (go = the launch), bring them to the host and split the `rows` device rows
// of 4 n_bins + 4 counters into the caller's three arrays (any of them may be NULL)
extern "C++" template <class Go>
static int texture_rows(Handle* h, hipStream_t st, int64_t rows, int nb, int64_t* gb_hist, int64_t* pole_hist, int64_t* bad, Go&& go)
{
    const int nc = 4 * nb + 4;
    DevTmp<unsigned long long> d_rows;
    HIPCHK(d_rows.alloc((size_t)rows * nc));
    HIPCHK(hipMemsetAsync(d_rows.p, 0, (size_t)rows * nc * sizeof(unsigned long long), st));
    go(d_rows.p);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> host((size_t)rows * nc);
    HIPCHK(hipMemcpyAsync(host.data(), d_rows.p, host.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    h->cnt.bytes_d2h += (int64_t)(host.size() * sizeof(int64_t));
    for (int64_t r = 0; r < rows; ++r) {
        const int64_t* s = host.data() + r * nc;
        if (gb_hist) std::copy(s, s + 3 * nb, gb_hist + r * 3 * nb);
        if (pole_hist) std::copy(s + 3 * nb, s + 4 * nb, pole_hist + r * nb);
        if (bad) std::copy(s + 4 * nb, s + nc, bad + r * 4);
    }
    return 0;
}

static int texture_profile(const char* fn, void* handle, bool ens, const struct cetkmc_texture_args* args, int64_t* gb_hist, int64_t* pole_hist,
                           int64_t* bad)
{
    if (!handle || !args) return fail("null argument");
    Lattices A;
    CHK(lattices(fn, handle, ens, ONE_LATTICE | CLUSTERS | VIEWS, &A));
    TexArgs T;
    CHK(texture_args(fn, args, &T));
    return texture_rows(A.h0, A.stream, (int64_t)A.R * A.L, T.n_bins, gb_hist, pole_hist, bad, [&](unsigned long long* d_rows) {
        A.run(ENS_LABELS, [&](auto... sel) {
            launch(k_texture_profile<decltype(sel)...>, texture_grid(A.L, A.R), dim3(256), 0, A.stream, nullptr, nullptr, A.view, A.labels, T, d_rows, sel...);
        });
    });
}
int cetkmc_texture_profile(void* handle, const struct cetkmc_texture_args* args, int64_t* gb_hist, int64_t* pole_hist, int64_t* bad)
{
    return texture_profile("cetkmc_texture_profile", handle, false, args, gb_hist, pole_hist, bad);
}
int cetkmc_ensemble_texture_profile(void* handle, const struct cetkmc_texture_args* args, int64_t* gb_hist, int64_t* pole_hist,
                                    int64_t* bad)
{
    return texture_profile("cetkmc_ensemble_texture_profile", handle, true, args, gb_hist, pole_hist, bad);
}


// ---- per-grain table (grain.hpp) ----------------------------------------------------------------
static unsigned grain_blocks(int L) { return (unsigned)(((int64_t)L * L * L + GRAIN_VPB - 1) / GRAIN_VPB); }

// cap: how many records the caller takes (the ensemble call: all of them)
static int grain_table(const char* fn, void* handle, bool ens, int64_t cap, struct cetkmc_grain_rec* out)
{
    if (!handle) return fail(ens ? "null argument" : "null handle");
    Lattices A;
    CHK(lattices(fn, handle, ens, ONE_LATTICE | CLUSTERS | VIEWS, &A));
    const int64_t nc = A.grains, n = std::min<int64_t>(cap, nc);
    if (n <= 0) return 0;
    if (!out) return fail("null argument");
    // the device table holds every grain (the pass adds by label); the first n records are the caller's
    return fill_records<unsigned long long>(A.h0, A.stream, "per-grain table", GRAIN_NW, nullptr, 0, nc, n, nullptr, out,
                                            [&](unsigned long long*, unsigned long long* d_rec) {
        A.run(ENS_GRAINS, [&](auto... sel) {
            launch(k_grain_table<decltype(sel)...>, dim3(grain_blocks(A.L), (unsigned)A.R), dim3(256), 0, A.stream, nullptr, nullptr, A.view, A.labels, A.n, d_rec,
                   sel...);
            launch(k_grain_first<decltype(sel)...>, A.grain_grid((A.max_grains + 255) / 256), dim3(256), 0, A.stream, nullptr, nullptr, A.view, A.roots, A.n,
                   d_rec, sel...);
        });
        return 0;
    });
}
int cetkmc_grain_table(void* handle, int64_t cap, struct cetkmc_grain_rec* out) { return grain_table("cetkmc_grain_table", handle, false, cap, out); }
int cetkmc_ensemble_grain_table(void* handle, struct cetkmc_grain_rec* out)
{
    return grain_table("cetkmc_ensemble_grain_table", handle, true, INT64_MAX, out);
}


// ---- solidification map (solid.hpp) -------------------------------------------------------------
// One device block for the maps of hs (one handle, or every replica of an ensemble): all stamps, then all doubles, the two
// snapshots, the counters [n][3] and the map table [n] -- so that begin sets the block with two memsets whatever n.
struct SolidLayout { size_t n, nsnap, o_dbl, o_snap, o_tsnap, o_cnt, o_tab, bytes; };
static SolidLayout solid_layout(int L, int pitchT, size_t R)
{
    SolidLayout y{};
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    y.n = (size_t)L * L * L; y.nsnap = (size_t)L * L * pitchT;
    y.o_dbl = up(R * y.n * 8);
    y.o_snap = y.o_dbl + up(R * y.n * 5 * 8);
    y.o_tsnap = y.o_snap + R * up(y.nsnap);
    y.o_cnt = y.o_tsnap + R * up(y.nsnap * 8);
    y.o_tab = y.o_cnt + up(R * 3 * 8);
    y.bytes = y.o_tab + up(R * sizeof(SolidMap));
    return y;
}
static dim3 solid_update_grid(int L, int pitchT, int R, int pairs_per_block)
{
    const int64_t npair = (int64_t)L * L * (pitchT / 2);
    return dim3((unsigned)((npair + pairs_per_block - 1) / pairs_per_block), (unsigned)R);
}
static unsigned solid_blocks(int L) { return (unsigned)(((int64_t)L * L * L + SOLID_VPB - 1) / SOLID_VPB); }

static int solid_update_args(const char* fn, int64_t stamp, double inv_dx, double dt)
{
    const std::string f(fn);
    if (stamp < 0) return fail(f + ": stamp " + std::to_string(stamp) + " is negative");
    if (!std::isfinite(dt) || !(dt > 0.0)) return fail(f + ": dt must be finite and > 0");
    if (!std::isfinite(inv_dx)) return fail(f + ": inv_dx is not finite");
    return 0;
}
static int solid_scales(const char* fn, const struct cetkmc_solid_args* a)
{
    for (int c = 0; c < 4; ++c)
        if (!std::isfinite(a->qscale[c]) || !(a->qscale[c] > 0.0)) return fail(std::string(fn) + ": qscale[" + std::to_string(c) + "] must be finite and > 0");
    return 0;
}

// the counters of n lattices behind an update -> info, and each handle's running record count
static int solid_collect(std::vector<Handle*>& hs, const unsigned long long* d_cnt, hipStream_t st, struct cetkmc_solid_info* info)
{
    std::vector<unsigned long long> c(3 * hs.size());
    HIPCHK(hipMemcpyAsync(c.data(), d_cnt, c.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    hs[0]->cnt.bytes_d2h += (int64_t)c.size() * 8;
    for (size_t r = 0; r < hs.size(); ++r) {
        hs[r]->solid_recorded += (int64_t)c[3 * r] - (int64_t)c[3 * r + 2];
        if (info) { info[r].n_new = (int64_t)c[3 * r]; info[r].n_cleared = (int64_t)c[3 * r + 1]; info[r].n_recorded = hs[r]->solid_recorded; }
    }
    return 0;
}

// the device table of the maps a launch indexes by replica (null: one lattice, its map goes by value)
static const SolidMap* solid_maps(const Lattices& A) { return A.e ? A.e->d_solid_maps : nullptr; }

// (re)start the maps of the pass's lattices in their block (allocated here if there is none)
static int solid_begin(const char* fn, void* handle, bool ens)
{
    Lattices A;
    CHK(lattices(fn, handle, ens, OWNER | SOLID | VIEWS, &A));
    Handle* h0 = A.h0;
    hipStream_t st = A.stream;
    void** block = A.e ? &A.e->d_solid_block : &h0->d_solid_block;
    const size_t R = (size_t)A.R;
    const SolidLayout y = solid_layout(A.L, h0->pitchT, R);
    if (!*block) {
        if (hipMalloc(block, y.bytes) != hipSuccess) {
            (void)hipGetLastError();
            *block = nullptr;
            return fail("solidification map: no device memory for " + std::to_string(y.bytes) + " bytes");
        }
    }
    // no handle has a map until everything below has completed: an error on the way leaves none (a second begin included)
    for (Handle* h : A.hs) { h->solid_on = false; h->solid_recorded = 0; }
    char* b = (char*)*block;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    std::vector<SolidMap> tab(R);
    for (size_t r = 0; r < R; ++r) {
        SolidMap& m = tab[r];
        m.stamp = (long long*)b + r * y.n;
        double* d = (double*)(b + y.o_dbl) + r * 5 * y.n;
        m.Ts = d; m.g = d + y.n; m.cool = d + 4 * y.n;
        m.snap = (uint8_t*)(b + y.o_snap + r * up(y.nsnap));
        m.Tsnap = (double*)(b + y.o_tsnap + r * up(y.nsnap * 8));
        m.cnt = (unsigned long long*)(b + y.o_cnt) + 3 * r;
        A.hs[r]->solid = m;
    }
    if (A.e) A.e->d_solid_maps = (SolidMap*)(b + y.o_tab);
    auto issue = [&]() -> int {
        HIPCHK(hipMemsetAsync(b, 0xff, R * y.n * 8, st));                           // stamp = -1
        HIPCHK(hipMemsetAsync(b + y.o_dbl, 0, y.bytes - y.o_dbl, st));               // +0.0, snapshots, counters, table
        HIPCHK(hipMemcpyAsync(b + y.o_tab, tab.data(), R * sizeof(SolidMap), hipMemcpyHostToDevice, st));
        A.run(ENS_VIEWS, [&](auto... sel) {
            launch(k_solid_snapshot<decltype(sel)...>, solid_update_grid(A.L, h0->pitchT, A.R, 256), dim3(256), 0, st, nullptr, nullptr, A.view, h0->solid,
                   solid_maps(A), sel...);
        });
        HIPCHK(hipGetLastError());
        return 0;
    };
    const int rc = issue();
    const hipError_t synced = hipStreamSynchronize(st);         // also after an error: the table is copied from this frame
    if (rc) return rc;
    HIPCHK(synced);
    for (Handle* h : A.hs) h->solid_on = true;
    return 0;
}
int cetkmc_solid_begin(void* handle) { return solid_begin("cetkmc_solid_begin", handle, false); }
int cetkmc_ensemble_solid_begin(void* handle) { return solid_begin("cetkmc_ensemble_solid_begin", handle, true); }

static int solid_end(const char* fn, void* handle, bool ens)
{
    Lattices A;
    CHK(lattices(fn, handle, ens, OWNER | SOLID, &A));
    void*& block = A.e ? A.e->d_solid_block : A.h0->d_solid_block;
    if (!block) return fail(no_map(fn, ens, SOLID));      // (a begin that failed half way keeps its block)
    HIPCHK(hipStreamSynchronize(A.stream));
    HIPCHK(hipFree(block));
    block = nullptr;
    if (A.e) A.e->d_solid_maps = nullptr;
    for (Handle* h : A.hs) { h->solid = SolidMap{}; h->solid_on = false; h->solid_recorded = 0; }
    return 0;
}
int cetkmc_solid_end(void* handle) { return solid_end("cetkmc_solid_end", handle, false); }
int cetkmc_ensemble_solid_end(void* handle) { return solid_end("cetkmc_ensemble_solid_end", handle, true); }

static int solid_update(const char* fn, void* handle, bool ens, int64_t stamp, double inv_dx, double dt, struct cetkmc_solid_info* info)
{
    Lattices A;
    CHK(lattices(fn, handle, ens, OWNER | SOLID | MAP | VIEWS, &A));
    CHK(solid_update_args(fn, stamp, inv_dx, dt));
    Handle* h0 = A.h0;
    HIPCHK(hipMemsetAsync(h0->solid.cnt, 0, (size_t)A.R * 3 * 8, A.stream));       // replica 0's counters head the block's [R][3]
    A.run(ENS_VIEWS, [&](auto... sel) {
        launch(k_solid_update<decltype(sel)...>, solid_update_grid(A.L, h0->pitchT, A.R, SOLID_PPB), dim3(256), 0, A.stream, nullptr, nullptr, A.view,
               h0->solid, solid_maps(A), (long long)stamp, inv_dx, dt, sel...);
    });
    HIPCHK(hipGetLastError());
    return solid_collect(A.hs, h0->solid.cnt, A.stream, info);
}
int cetkmc_solid_update(void* handle, int64_t stamp, double inv_dx, double dt, struct cetkmc_solid_info* info)
{
    return solid_update("cetkmc_solid_update", handle, false, stamp, inv_dx, dt, info);
}
int cetkmc_ensemble_solid_update(void* handle, int64_t stamp, double inv_dx, double dt, struct cetkmc_solid_info* info)
{
    return solid_update("cetkmc_ensemble_solid_update", handle, true, stamp, inv_dx, dt, info);
}


int cetkmc_solid_read(void* handle, int64_t* stamp, double* T_s, double* g, double* cool)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    if (h->slabs.size() != 1 || h->nranks != 1) return fail("cetkmc_solid_read needs the whole lattice in one slab");
    if (!h->solid_on) return fail("cetkmc_solid_read needs a map (cetkmc_solid_begin)");
    HIPCHK(hipSetDevice(h->dev));
    const size_t n = (size_t)h->L * h->L * h->L;
    int64_t bytes = 0;
    if (stamp) { HIPCHK(hipMemcpyAsync(stamp, h->solid.stamp, n * 8, hipMemcpyDeviceToHost, h->stream)); bytes += (int64_t)n * 8; }
    if (T_s) { HIPCHK(hipMemcpyAsync(T_s, h->solid.Ts, n * 8, hipMemcpyDeviceToHost, h->stream)); bytes += (int64_t)n * 8; }
    if (g) { HIPCHK(hipMemcpyAsync(g, h->solid.g, n * 24, hipMemcpyDeviceToHost, h->stream)); bytes += (int64_t)n * 24; }
    if (cool) { HIPCHK(hipMemcpyAsync(cool, h->solid.cool, n * 8, hipMemcpyDeviceToHost, h->stream)); bytes += (int64_t)n * 8; }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cnt.bytes_d2h += bytes;
    return 0;
}

// cap: how many grain records the caller takes (the ensemble call: all of them)
static int solid_profile(const char* fn, void* handle, bool ens, const struct cetkmc_solid_args* args, struct cetkmc_solid_rec* layers, int64_t cap,
                         struct cetkmc_solid_rec* grains)
{
    const bool outputs = args && layers;      // the single call asks for them first, the ensemble call for its maps
    if (!ens && !outputs) return fail("null argument");
    Lattices A;
    CHK(lattices(fn, handle, ens, ONE_LATTICE | SOLID | MAP, &A));
    if (!outputs) return fail("null argument");
    CHK(solid_scales(fn, args));
    if (grains && A.grains < 0) return fail(no_clusters(fn, ens) + " for its grain records");
    const int64_t nc = grains ? A.grains : 0, n = std::min<int64_t>(cap, nc);
    const bool with_grains = grains && n > 0;
    // the device table holds every grain (the pass adds by label); the first n records are the caller's
    return fill_records<long long>(A.h0, A.stream, "solidification profile", SOLID_NW, k_solid_rec_init, (int64_t)A.R * A.L, with_grains ? nc : 0,
                                   with_grains ? n : 0, layers, grains, [&](long long* d_lay, long long* d_gr) {
        A.run(ENS_GRAINS, [&](auto... sel) {
            launch(k_solid_profile<decltype(sel)...>, dim3(solid_blocks(A.L), (unsigned)A.R), dim3(256), 0, A.stream, nullptr, nullptr, A.h0->solid,
                   solid_maps(A), A.L, with_grains ? A.labels : nullptr, grains ? A.n : 0, args->qscale[0], args->qscale[1], args->qscale[2], args->qscale[3],
                   d_lay, d_gr, sel...);
        });
        return 0;
    });
}
int cetkmc_solid_profile(void* handle, const struct cetkmc_solid_args* args, struct cetkmc_solid_rec* layers, int64_t cap,
                         struct cetkmc_solid_rec* grains)
{
    return solid_profile("cetkmc_solid_profile", handle, false, args, layers, cap, grains);
}
int cetkmc_ensemble_solid_profile(void* handle, const struct cetkmc_solid_args* args, struct cetkmc_solid_rec* layers,
                                  struct cetkmc_solid_rec* grains)
{
    return solid_profile("cetkmc_ensemble_solid_profile", handle, true, args, layers, INT64_MAX, grains);
}


// ---- origin map (origin.hpp) --------------------------------------------------------------------
// One device block for the maps of hs (one handle, or every replica of an ensemble): all words, all censuses, the map table
// [n] and the run table [n] -- so that begin clears the block with one memset whatever n.
struct OriginLayout { size_t n, o_census, o_tab, o_runs, bytes; };
static OriginLayout origin_layout(int L, size_t R)
{
    OriginLayout y{};
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    y.n = (size_t)L * L * L;
    y.o_census = up(R * y.n * 8);
    y.o_tab = y.o_census + up(R * (size_t)L * 5 * 8);
    y.o_runs = y.o_tab + up(R * sizeof(OriginMap));
    y.bytes = y.o_runs + up(R * sizeof(OriginRun));
    return y;
}
static unsigned origin_blocks(int L) { return (unsigned)(((int64_t)L * L * L + ORIGIN_VPB - 1) / ORIGIN_VPB); }

// (re)start the maps of the pass's lattices in their block (allocated here if there is none); max_L: the single call's limit
static int origin_begin(const char* fn, void* handle, bool ens, int max_L)
{
    Lattices A;
    CHK(lattices(fn, handle, ens, OWNER | ORIGIN, &A));
    for (Handle* h : A.hs)
        if (h->ts.remelt_on) return fail(std::string(fn) + " is refused while remelting is on: the event log the origin map folds holds no melts");
    if (A.L > max_L) return fail(std::string(fn) + ": L > " + std::to_string(max_L) + " (the profile packs a voxel's linear index into 24 bits)");
    void** block = A.e ? &A.e->d_origin_block : &A.h0->d_origin_block;
    const size_t R = (size_t)A.R;
    const OriginLayout y = origin_layout(A.L, R);
    if (!*block) {
        if (hipMalloc(block, y.bytes) != hipSuccess) {
            (void)hipGetLastError();
            *block = nullptr;
            return fail("origin map: no device memory for " + std::to_string(y.bytes) + " bytes");
        }
    }
    // no handle has a map until everything below has completed: an error on the way leaves none (a second begin included)
    for (Handle* h : A.hs) { h->origin_on = false; h->origin_seq = 0; }
    char* b = (char*)*block;
    std::vector<OriginMap> tab(R);
    for (size_t r = 0; r < R; ++r) {
        tab[r].words = (unsigned long long*)b + r * y.n;
        tab[r].census = (long long*)(b + y.o_census) + r * (size_t)A.L * 5;
        A.hs[r]->origin = tab[r];
    }
    if (A.e) { A.e->d_origin_maps = (OriginMap*)(b + y.o_tab); A.e->d_origin_runs = (OriginRun*)(b + y.o_runs); }
    auto issue = [&]() -> int {
        HIPCHK(hipMemsetAsync(b, 0, y.bytes, A.stream));
        HIPCHK(hipMemcpyAsync(b + y.o_tab, tab.data(), R * sizeof(OriginMap), hipMemcpyHostToDevice, A.stream));
        return 0;
    };
    const int rc = issue();
    const hipError_t synced = hipStreamSynchronize(A.stream);         // also after an error: the table is copied from this frame
    if (rc) return rc;
    HIPCHK(synced);
    for (Handle* h : A.hs) h->origin_on = true;
    return 0;
}
int cetkmc_origin_begin(void* handle) { return origin_begin("cetkmc_origin_begin", handle, false, 256); }
int cetkmc_ensemble_origin_begin(void* handle) { return origin_begin("cetkmc_ensemble_origin_begin", handle, true, INT_MAX); }

static int origin_end(const char* fn, void* handle, bool ens)
{
    Lattices A;
    CHK(lattices(fn, handle, ens, OWNER | ORIGIN, &A));
    void*& block = A.e ? A.e->d_origin_block : A.h0->d_origin_block;
    if (!block) return fail(no_map(fn, ens, ORIGIN));      // (a begin that failed half way keeps its block)
    HIPCHK(hipStreamSynchronize(A.stream));
    HIPCHK(hipFree(block));
    block = nullptr;
    if (A.e) { A.e->d_origin_maps = nullptr; A.e->d_origin_runs = nullptr; }
    for (Handle* h : A.hs) { h->origin = OriginMap{}; h->origin_on = false; h->origin_seq = 0; }
    return 0;
}
int cetkmc_origin_end(void* handle) { return origin_end("cetkmc_origin_end", handle, false); }
int cetkmc_ensemble_origin_end(void* handle) { return origin_end("cetkmc_ensemble_origin_end", handle, true); }

int64_t cetkmc_origin_seq(void* handle)
{
    Handle* h = (Handle*)handle;
    return (h && h->origin_on) ? h->origin_seq : -1;
}

int cetkmc_origin_absorb_events(void* handle, const cetkmc_event* ev, int64_t n, int64_t group)
{
    Handle* h = (Handle*)handle;
    Lattices A;
    CHK(lattices("cetkmc_origin_absorb_events", handle, false, ORIGIN | MAP, &A));
    if (n < 0) return fail("cetkmc_origin_absorb_events: n < 0");
    if (group < 1) return fail("cetkmc_origin_absorb_events: group must be >= 1");
    if (n % group) return fail("cetkmc_origin_absorb_events: n must be a multiple of group");
    if (n > 0 && !ev) return fail("null argument");
    const int L = h->L;
    for (int64_t q = 0; q < n; ++q) {
        const cetkmc_event& r = ev[q];
        if (r.type < 0 || r.type > 3) continue;
        for (int c = 0; c < 3; ++c)
            if (r.pos[c] < 0 || r.pos[c] >= L) return fail("cetkmc_origin_absorb_events: record " + std::to_string(q) + ": position outside the lattice");
        if (r.type == CETKMC_DIFF && r.target[0] >= 0)
            for (int c = 0; c < 3; ++c)
                if (r.target[c] < 0 || r.target[c] >= L) return fail("cetkmc_origin_absorb_events: record " + std::to_string(q) + ": diffusion target outside the lattice");
    }
    CHK(origin_room(h, n / group, "cetkmc_origin_absorb_events"));
    if (n == 0) return 0;
    DevTmp<cetkmc_event> d_ev;
    if (d_ev.alloc((size_t)n) != hipSuccess) {
        (void)hipGetLastError();
        return fail("cetkmc_origin_absorb_events: no device memory for " + std::to_string(n) + " records");
    }
    HIPCHK(hipMemcpyAsync(d_ev.p, ev, (size_t)n * sizeof(cetkmc_event), hipMemcpyHostToDevice, h->stream));
    h->cnt.bytes_h2d += n * (int64_t)sizeof(cetkmc_event);
    CHK(origin_absorb_log(h, d_ev.p, n, group));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

int cetkmc_origin_read(void* handle, uint64_t* words)
{
    Handle* h = (Handle*)handle;
    if (!words) return fail("null argument");
    Lattices A;
    CHK(lattices("cetkmc_origin_read", handle, false, ORIGIN | MAP, &A));
    const size_t n = (size_t)h->L * h->L * h->L;
    HIPCHK(hipMemcpyAsync(words, h->origin.words, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->cnt.bytes_d2h += (int64_t)n * 8;
    return 0;
}

static int origin_census(const char* fn, void* handle, bool ens, int64_t* out)
{
    if (!ens && !out) return fail("null argument");      // the single call asks for its output first, the ensemble call for its maps
    Lattices A;
    CHK(lattices(fn, handle, ens, ORIGIN | MAP, &A));
    if (!out) return fail("null argument");
    const size_t bytes = (size_t)A.R * A.L * 5 * 8;       // replica 0's census heads the block's [R][L][5]
    HIPCHK(hipMemcpyAsync(out, A.h0->origin.census, bytes, hipMemcpyDeviceToHost, A.stream));
    HIPCHK(hipStreamSynchronize(A.stream));
    A.h0->cnt.bytes_d2h += (int64_t)bytes;
    return 0;
}
int cetkmc_origin_census(void* handle, int64_t* out) { return origin_census("cetkmc_origin_census", handle, false, out); }
int cetkmc_ensemble_origin_census(void* handle, int64_t* out) { return origin_census("cetkmc_ensemble_origin_census", handle, true, out); }

// cap: how many grain records the caller takes (the ensemble call: all of them)
static int origin_profile(const char* fn, void* handle, bool ens, struct cetkmc_origin_rec* layers, int64_t cap, struct cetkmc_origin_rec* grains)
{
    if (!ens && !layers) return fail("null argument");   // as in origin_census
    Lattices A;
    CHK(lattices(fn, handle, ens, ONE_LATTICE | ORIGIN | MAP, &A));
    if (!layers) return fail("null argument");
    if (grains && A.grains < 0) return fail(no_clusters(fn, ens) + " for its grain records");
    const int64_t nc = grains ? A.grains : 0, n = std::min<int64_t>(cap, nc);
    const bool with_grains = grains && n > 0;
    // the device table holds every grain (the pass adds by label); the first n records are the caller's
    return fill_records<long long>(A.h0, A.stream, "origin profile", ORIGIN_NW, k_origin_rec_init, (int64_t)A.R * A.L, with_grains ? nc : 0,
                                   with_grains ? n : 0, layers, grains, [&](long long* d_lay, long long* d_gr) {
        if (A.e) CHK(ens_push_views(A.e));      // the pass reads every replica's state through its current view
        A.run(ENS_GRAINS, [&](auto... sel) {
            launch(k_origin_profile<decltype(sel)...>, dim3(origin_blocks(A.L), (unsigned)A.R), dim3(256), 0, A.stream, nullptr, nullptr, A.view,
                   A.h0->origin, A.e ? A.e->d_origin_maps : nullptr, with_grains ? A.labels : nullptr, grains ? A.n : 0, d_lay, d_gr, sel...);
        });
        return 0;
    });
}
int cetkmc_origin_profile(void* handle, struct cetkmc_origin_rec* layers, int64_t cap, struct cetkmc_origin_rec* grains)
{
    return origin_profile("cetkmc_origin_profile", handle, false, layers, cap, grains);
}
int cetkmc_ensemble_origin_profile(void* handle, struct cetkmc_origin_rec* layers, struct cetkmc_origin_rec* grains)
{
    return origin_profile("cetkmc_ensemble_origin_profile", handle, true, layers, INT64_MAX, grains);
}

// ---- remelting (melt.hpp) -----------------------------------------------------------------------
// The setters of ThermalSettings, each written once for a single handle (cetkmc_set_X) and for an ensemble (ens,
// cetkmc_ensemble_set_X; its handle is replica 0's).  fn names the entry point, prefix_of(ens) + "set_Y" a setter for the same
// kind of handle, other_kind(fn, ens) the entry point's counterpart.
static std::string prefix_of(bool ens) { return ens ? "cetkmc_ensemble_" : "cetkmc_"; }
static std::string other_kind(const char* fn, bool ens) { return prefix_of(!ens) + (fn + prefix_of(ens).size()); }
// how the setters but cetkmc_set_remelt open: the ensemble of an ensemble handle, and the handle kind the entry point is not for
static int setter_ensemble(const char* fn, void* handle, bool ens, Ens** e)
{
    *e = ens_of(handle);
    if (ens && !*e) return fail(std::string(fn) + ": not an ensemble handle (cetkmc_create_ensemble)");
    if (!ens && *e) return fail(std::string(fn) + ": an ensemble handle is set by " + other_kind(fn, ens));
    return 0;
}
// the record a setter writes: the ensemble's (handed on to every replica by share_thermal), or the handle's own
static ThermalSettings& settings_of(Handle* h, Ens* e) { return e ? e->ts : h->ts; }

// every replica's row flags and counters, and the device table that names them [R]
static int ens_melt_ensure(Ens* e, const char* fn)
{
    const size_t R = (size_t)e->R;
    Handle* h0 = e->reps[0];
    for (Handle* h : e->reps) CHK(melt_ensure(h));
    if (e->d_melt_tab) return 0;
    if (hipMalloc((void**)&e->d_melt_tab, R * sizeof(MeltState)) != hipSuccess || hipMalloc((void**)&e->d_melt_out, R * 4 * 8) != hipSuccess) {
        (void)hipGetLastError();
        if (e->d_melt_tab) (void)hipFree(e->d_melt_tab);
        e->d_melt_tab = nullptr; e->d_melt_out = nullptr;
        return fail(std::string(fn) + ": no device memory for the replica table");
    }
    std::vector<MeltState> tab(R);
    for (size_t r = 0; r < R; ++r) tab[r] = e->reps[r]->melt;
    HIPCHK(hipMemcpyAsync(e->d_melt_tab, tab.data(), R * sizeof(MeltState), hipMemcpyHostToDevice, h0->stream));
    HIPCHK(hipStreamSynchronize(h0->stream));       // the table is copied from this frame
    return 0;
}
static int set_remelt(const char* fn, void* handle, bool ens, int on, double threshold)
{
    const std::string f(fn);
    if (!handle) return fail(ens ? "null argument" : "null handle");
    Ens* e = ens ? ens_of(handle) : nullptr;
    if (ens && !e) return fail(f + ": not an ensemble handle (cetkmc_create_ensemble)");
    Handle* h = (Handle*)handle;
    CHK(melt_refusals(h, fn, threshold));
    if (!ens && h->in_ensemble) return fail(f + ": the replicas of an ensemble are switched by " + other_kind(fn, ens));
    if (on && h->origin_on)
        return fail(f + (ens ? " is refused while the origin maps are attached: the event log they fold holds no melts"
                             : " is refused while an origin map is attached: the event log it folds holds no melts"));
    if (!ens && on && h->thermal_ahead) return fail(f + " is refused with option thermal_lookahead on (the field computed ahead knows no melt)");
    HIPCHK(hipSetDevice(h->dev));
    if (on) CHK(ens ? ens_melt_ensure(e, fn) : melt_ensure(h));
    ThermalSettings& s = settings_of(h, e);
    s.remelt_on = on ? 1 : 0;
    s.remelt_threshold = threshold;
    if (e) share_thermal(e);
    return 0;
}
int cetkmc_set_remelt(void* handle, int on, double threshold) { return set_remelt("cetkmc_set_remelt", handle, false, on, threshold); }
int cetkmc_ensemble_set_remelt(void* handle, int on, double threshold) { return set_remelt("cetkmc_ensemble_set_remelt", handle, true, on, threshold); }

int cetkmc_remelt(void* handle, double threshold, struct cetkmc_remelt_info* info)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("null handle");
    CHK(melt_refusals(h, "cetkmc_remelt", threshold));
    if (h->origin_on) return fail("cetkmc_remelt is refused while an origin map is attached: the event log it folds holds no melts");
    HIPCHK(hipSetDevice(h->dev));
    CHK(melt_ensure(h));
    CHK(launch_melt(h, threshold, false));
    unsigned long long c[4];
    int n_list = 0;
    HIPCHK(hipMemcpyAsync(c, h->melt.cnt, sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&n_list, h->slabs[0].v.ifc_n, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    melt_info_from(h, c);
    grow_ifc_grid(h, n_list);               // the list may have grown, as after an upload
    invalidate(h, Cause::apply);            // touched voxels relisted, not evaluated
    if (info) *info = h->melt_info;
    return 0;
}

int cetkmc_time_remelt(void* handle, double threshold, int n, double* ms_total)
{
    Handle* h = (Handle*)handle;
    if (!h || !ms_total) return fail("null argument");
    CHK(melt_refusals(h, "cetkmc_time_remelt", threshold));
    if (h->origin_on) return fail("cetkmc_time_remelt is refused while an origin map is attached: the event log it folds holds no melts");
    HIPCHK(hipSetDevice(h->dev));
    CHK(melt_ensure(h));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    for (int s = 0; s < n; ++s) CHK(launch_melt(h, threshold, false));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    cetkmc_remelt_info info;
    CHK(cetkmc_remelt(handle, threshold, &info));      // one more pass, untimed: reads the counters, grows the grid, names the cause
    *ms_total = 0.0;
    return add_elapsed(h->ev0, h->ev1, ms_total);
}

int cetkmc_get_remelt_info(void* handle, struct cetkmc_remelt_info* info)
{
    Handle* h = (Handle*)handle;
    if (!h || !info) return fail("null argument");
    *info = h->melt_info;
    return 0;
}

int cetkmc_ensemble_remelt_info(void* handle, struct cetkmc_remelt_info* info)
{
    if (!handle || !info) return fail("null argument");
    Ens* e = ens_of(handle);
    if (!e) return fail("cetkmc_ensemble_remelt_info: not an ensemble handle (cetkmc_create_ensemble)");
    for (int r = 0; r < e->R; ++r) info[r] = e->reps[(size_t)r]->melt_info;
    return 0;
}

// ---- sub-stepped temperature updates (thermal_sub.hpp) --------------------------------------------
static int substeps_range(const char* fn, int n)
{
    if (n < 1) return fail(std::string(fn) + ": thermal_substeps must be >= 1 (got " + std::to_string(n) + ")");
    if (n > CETKMC_MAX_THERMAL_SUBSTEPS)
        return fail(std::string(fn) + ": thermal_substeps above " + std::to_string(CETKMC_MAX_THERMAL_SUBSTEPS) + " (the launch bookkeeping is int)");
    return 0;
}

static int set_thermal_substeps(const char* fn, void* handle, bool ens, int n)
{
    const std::string f(fn);
    if (!handle) return fail(ens ? "null argument" : "null handle");
    Ens* e = nullptr;
    CHK(setter_ensemble(fn, handle, ens, &e));
    Handle* h = (Handle*)handle;
    CHK(substeps_range(fn, n));
    if (!ens) {
        if (h->in_ensemble) return fail(f + ": the replicas of an ensemble share one value (" + other_kind(fn, ens) + ")");
        if (multi_rank(h) || h->nranks != 1) return fail(f + " is refused on a rank handle (cetkmc_create_rank*): the halo exchange carries two planes per update");
        if (n > 1 && h->thermal_ahead) return fail(f + ": n > 1 is refused with option thermal_lookahead on (the field computed ahead is one explicit step)");
    }
    settings_of(h, e).substeps = n;
    if (e) share_thermal(e);
    return 0;
}
int cetkmc_set_thermal_substeps(void* handle, int n) { return set_thermal_substeps("cetkmc_set_thermal_substeps", handle, false, n); }
int cetkmc_ensemble_set_thermal_substeps(void* handle, int n) { return set_thermal_substeps("cetkmc_ensemble_set_thermal_substeps", handle, true, n); }

// the records of an ensemble handle are the ensemble's (replica 0's own cannot be read), any other handle's are its own
static const ThermalInfo& thermal_info_of(void* handle)
{
    Ens* e = ens_of(handle);
    return e ? e->ti : ((Handle*)handle)->ti;
}
int cetkmc_get_substep_info(void* handle, struct cetkmc_substep_info* info)
{
    if (!handle || !info) return fail("null argument");
    *info = thermal_info_of(handle).sub;
    return 0;
}

int cetkmc_time_thermal(void* handle, int laser, int n_updates, double* ms_total)
{
    if (!handle || !ms_total) return fail("null argument");
    if (ens_of(handle)) return fail("cetkmc_time_thermal: a single handle (an ensemble's updates run inside cetkmc_run_ensemble)");
    Handle* h = (Handle*)handle;
    if (n_updates < 0) return fail("cetkmc_time_thermal: n_updates must be >= 0");
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    const bool beam = laser && h->ts.beam.on;       // a beam: row 0 of its table, update ordinal u0
    for (int u = 0; u < n_updates; ++u)
        CHK(launch_thermal(h, 1e-6, laser ? 1 : 0, laser && !beam ? h->d_qtop : nullptr, laser ? 1 : 0, 1, false, beam ? h->ts.beam.u0 : 0));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *ms_total = 0.0;
    return add_elapsed(h->ev0, h->ev1, ms_total);
}

// ---- implicit temperature updates (thermal_imp.hpp) ------------------------------------------------
static int scheme_known(const char* fn, int scheme)
{
    if (scheme != CETKMC_THERMAL_EXPLICIT && scheme != CETKMC_THERMAL_IMPLICIT)
        return fail(std::string(fn) + ": unknown thermal scheme " + std::to_string(scheme) + " (CETKMC_THERMAL_EXPLICIT = 0, CETKMC_THERMAL_IMPLICIT = 1)");
    return 0;
}

static int set_thermal_scheme(const char* fn, void* handle, bool ens, int scheme)
{
    const std::string f(fn), pre = prefix_of(ens);
    if (!handle) return fail(ens ? "null argument" : "null handle");
    Ens* e = nullptr;
    if (!ens) CHK(scheme_known(fn, scheme));        // (a single handle hears of an unknown scheme first, an ensemble of its handle)
    CHK(setter_ensemble(fn, handle, ens, &e));
    if (ens) CHK(scheme_known(fn, scheme));
    Handle* h = (Handle*)handle;
    if (!ens) {
        if (h->in_ensemble) return fail(f + ": the replicas of an ensemble share one scheme (" + other_kind(fn, ens) + ")");
        if (scheme == CETKMC_THERMAL_IMPLICIT) {
            CHK(one_slab_only(h, f + ": the implicit scheme", " (the solve along the plane axis crosses slabs)"));
            if (h->thermal_ahead) return fail(f + ": the implicit scheme is refused with option thermal_lookahead on (the field computed ahead is one explicit step)");
        }
    }
    ThermalSettings& s = settings_of(h, e);
    if (scheme == CETKMC_THERMAL_EXPLICIT && s.bc_on)
        return fail(f + ": the explicit scheme is refused while a thermal boundary is set (" + pre + "set_thermal_boundary(handle, NULL) first)");
    if (scheme == CETKMC_THERMAL_EXPLICIT && s.beam.on)
        return fail(f + ": the explicit scheme is refused while a beam is set (" + pre + "set_beam with NULL first); the explicit kernels read a source plane");
    s.scheme = scheme;
    if (e) share_thermal(e);
    return 0;
}
int cetkmc_set_thermal_scheme(void* handle, int scheme) { return set_thermal_scheme("cetkmc_set_thermal_scheme", handle, false, scheme); }
int cetkmc_ensemble_set_thermal_scheme(void* handle, int scheme) { return set_thermal_scheme("cetkmc_ensemble_set_thermal_scheme", handle, true, scheme); }

int cetkmc_get_implicit_info(void* handle, struct cetkmc_implicit_info* info)
{
    if (!handle || !info) return fail("null argument");
    *info = thermal_info_of(handle).imp;
    return 0;
}

int cetkmc_implicit_coeffs(int L, double r, double* inv, double* p) { return implicit_coeffs_bc_host("cetkmc_implicit_coeffs", L, r, 0.0, 0.0, inv, p); }

// ---- thermal boundary conditions (thermal_imp.hpp) --------------------------------------------------
static int set_thermal_boundary(const char* fn, void* handle, bool ens, const cetkmc_thermal_boundary* b)
{
    const std::string f(fn), pre = prefix_of(ens);
    if (!handle) return fail(f + ": null handle");
    Ens* e = nullptr;
    CHK(setter_ensemble(fn, handle, ens, &e));
    Handle* h = (Handle*)handle;
    if (!ens && h->in_ensemble) return fail(f + ": the replicas of an ensemble share one boundary (" + other_kind(fn, ens) + ")");
    const cetkmc_thermal_boundary v = b ? *b : cetkmc_thermal_boundary{};
    CHK(boundary_values_ok(fn, v));
    const bool on = boundary_active(v);
    ThermalSettings& s = settings_of(h, e);
    if (on && s.scheme != CETKMC_THERMAL_IMPLICIT)
        return fail(f + ": a thermal boundary needs the implicit scheme (" + pre + "set_thermal_scheme); the explicit kernels are adiabatic");
    s.bc = v; s.bc_on = on;
    if (e) share_thermal(e);
    return 0;
}
int cetkmc_set_thermal_boundary(void* handle, const struct cetkmc_thermal_boundary* b) { return set_thermal_boundary("cetkmc_set_thermal_boundary", handle, false, b); }
int cetkmc_ensemble_set_thermal_boundary(void* handle, const struct cetkmc_thermal_boundary* b)
{
    return set_thermal_boundary("cetkmc_ensemble_set_thermal_boundary", handle, true, b);
}

int cetkmc_get_thermal_boundary(void* handle, struct cetkmc_thermal_boundary* b, struct cetkmc_boundary_info* info)
{
    if (!handle) return fail("cetkmc_get_thermal_boundary: null handle");
    Ens* e = ens_of(handle);
    if (b) *b = settings_of((Handle*)handle, e).bc;
    if (info) *info = (e ? e->ti : ((Handle*)handle)->ti).bc;
    return 0;
}

int cetkmc_implicit_coeffs_bc(int L, double r, double beta_lo, double beta_hi, double* inv, double* p)
{
    return implicit_coeffs_bc_host("cetkmc_implicit_coeffs_bc", L, r, beta_lo, beta_hi, inv, p);
}

// ---- beam tables: laser scan paths and a volumetric source (thermal_imp.hpp) --------------------------
static int beam_table_ok(const std::string& f, const cetkmc_beam& t, int L, const std::string& which)
{
    if (t.n_u < 1) return fail(f + ": " + which + "n_u must be >= 1 (got " + std::to_string(t.n_u) + ")");
    if (t.depth < 1 || t.depth > L) return fail(f + ": " + which + "depth must be in 1.." + std::to_string(L) + " (got " + std::to_string(t.depth) + ")");
    if (!t.amp || !t.gj || !t.gk || !t.fi) return fail(f + ": " + which + "amp, gj, gk and fi are required");
    struct Arr { const char* name; const double* p; int64_t n; };
    const Arr arrs[4] = {{"amp", t.amp, t.n_u}, {"gj", t.gj, (int64_t)t.n_u * L}, {"gk", t.gk, (int64_t)t.n_u * L}, {"fi", t.fi, t.depth}};
    for (const Arr& a : arrs)
        for (int64_t q = 0; q < a.n; ++q)
            if (!(a.p[q] >= 0.0) || !std::isfinite(a.p[q]))
                return fail(f + ": " + which + a.name + "[" + std::to_string(q) + "] is negative or not finite");
    return 0;
}
// one set behind the other in the layout BeamView names
static void beam_pack(const cetkmc_beam& t, int L, double* out)
{
    const size_t nu = (size_t)t.n_u, nl = nu * (size_t)L;
    memcpy(out, t.amp, nu * 8); memcpy(out + nu, t.gj, nl * 8); memcpy(out + nu + nl, t.gk, nl * 8); memcpy(out + nu + 2 * nl, t.fi, (size_t)t.depth * 8);
}
static int64_t beam_stride(const cetkmc_beam& t, int L) { return (int64_t)t.n_u * (1 + 2 * (int64_t)L) + t.depth; }
// the packed sets (and an ensemble's set_of) replace the table *d_tab / *d_set names; the launches that read the old one are awaited
static int beam_upload(const std::string& f, Handle* h, const std::vector<double>& tab, const int32_t* set_of, int R, double** d_tab, int32_t** d_set)
{
    HIPCHK(hipSetDevice(h->dev));
    double* nd = nullptr;
    int32_t* ns = nullptr;
    if (hipMalloc((void**)&nd, tab.size() * 8) != hipSuccess || (set_of && hipMalloc((void**)&ns, (size_t)R * 4) != hipSuccess)) {
        (void)hipGetLastError();
        if (nd) (void)hipFree(nd);
        return fail(f + ": no device memory for " + std::to_string(tab.size() * 8) + " bytes");
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(nd, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    if (set_of) HIPCHK(hipMemcpy(ns, set_of, (size_t)R * 4, hipMemcpyHostToDevice));
    if (*d_tab) (void)hipFree(*d_tab);
    *d_tab = nd;
    if (d_set) { if (*d_set) (void)hipFree(*d_set); *d_set = ns; }
    return 0;
}
static int beam_drop(Handle* h, double** d_tab, int32_t** d_set)
{
    if (!*d_tab) return 0;
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipStreamSynchronize(h->stream));
    (void)hipFree(*d_tab); *d_tab = nullptr;
    if (d_set && *d_set) { (void)hipFree(*d_set); *d_set = nullptr; }
    return 0;
}

int cetkmc_set_beam(void* handle, const struct cetkmc_beam* t)
{
    const std::string f = "cetkmc_set_beam";
    if (!handle) return fail(f + ": null handle");
    Ens* e = nullptr;
    CHK(setter_ensemble(f.c_str(), handle, false, &e));
    Handle* h = (Handle*)handle;
    if (h->in_ensemble) return fail(f + ": the replicas of an ensemble read the ensemble's table (cetkmc_ensemble_set_beam)");
    if (!t) {
        h->ts.beam = BeamView{};
        return beam_drop(h, &h->d_beam, nullptr);
    }
    CHK(beam_table_ok(f, *t, h->L, ""));
    if (h->ts.scheme != CETKMC_THERMAL_IMPLICIT)
        return fail(f + ": a beam needs the implicit scheme (cetkmc_set_thermal_scheme); the explicit kernels read a source plane");
    std::vector<double> tab((size_t)beam_stride(*t, h->L));
    beam_pack(*t, h->L, tab.data());
    CHK(beam_upload(f, h, tab, nullptr, 0, &h->d_beam, nullptr));
    BeamView& b = h->ts.beam;
    b = BeamView{};
    b.on = true; b.d = h->d_beam; b.u0 = t->u0; b.n_u = t->n_u; b.depth = t->depth; b.L = h->L; b.set_stride = (int64_t)tab.size();
    ++h->ti.beam.table_uploads;
    return 0;
}

int cetkmc_ensemble_set_beam(void* handle, int n_sets, const struct cetkmc_beam* sets, const int32_t* set_of)
{
    const std::string f = "cetkmc_ensemble_set_beam";
    if (!handle) return fail(f + ": null handle");
    Ens* e = nullptr;
    CHK(setter_ensemble(f.c_str(), handle, true, &e));
    Handle* h0 = e->reps[0];
    if (!sets) {
        e->ts.beam = BeamView{};
        share_thermal(e);
        return beam_drop(h0, &e->d_beam, &e->d_beam_set_of);
    }
    if (n_sets < 1) return fail(f + ": n_sets must be >= 1");
    for (int q = 0; q < n_sets; ++q) CHK(beam_table_ok(f, sets[q], e->L, "set " + std::to_string(q) + ": "));
    for (int q = 1; q < n_sets; ++q)
        if (sets[q].u0 != sets[0].u0 || sets[q].n_u != sets[0].n_u || sets[q].depth != sets[0].depth)
            return fail(f + ": set " + std::to_string(q) + " differs from set 0 in u0, n_u or depth (the sets share them)");
    if (!set_of && n_sets != e->R) return fail(f + ": set_of NULL means set r for replica r, so n_sets must equal R");
    std::vector<int32_t> so((size_t)e->R);
    for (int r = 0; r < e->R; ++r) {
        so[(size_t)r] = set_of ? set_of[r] : r;
        if (so[(size_t)r] < 0 || so[(size_t)r] >= n_sets) return fail(f + ": set_of[" + std::to_string(r) + "] is outside [0, n_sets)");
    }
    if (e->ts.scheme != CETKMC_THERMAL_IMPLICIT)
        return fail(f + ": a beam needs the implicit scheme (cetkmc_ensemble_set_thermal_scheme); the explicit kernels read a source plane");
    const int64_t stride = beam_stride(sets[0], e->L);
    std::vector<double> tab((size_t)stride * (size_t)n_sets);
    for (int q = 0; q < n_sets; ++q) beam_pack(sets[q], e->L, tab.data() + (size_t)q * (size_t)stride);
    CHK(beam_upload(f, h0, tab, so.data(), e->R, &e->d_beam, &e->d_beam_set_of));
    e->beam_set_of = so;
    BeamView& b = e->ts.beam;
    b = BeamView{};
    b.on = true; b.d = e->d_beam; b.set_of = e->d_beam_set_of; b.u0 = sets[0].u0; b.n_u = sets[0].n_u; b.depth = sets[0].depth; b.L = e->L; b.set_stride = stride;
    share_thermal(e);
    ++e->ti.beam.table_uploads;
    return 0;
}

int cetkmc_get_beam_info(void* handle, struct cetkmc_beam_info* info)
{
    if (!handle || !info) return fail("cetkmc_get_beam_info: null argument");
    *info = thermal_info_of(handle).beam;
    return 0;
}

int cetkmc_thermal_beam(void* handle, double dt, int64_t u, int use_latent, int scrub_nan)
{
    Handle* h = (Handle*)handle;
    if (!h) return fail("cetkmc_thermal_beam: null handle");
    if (!h->ts.beam.on) return fail("cetkmc_thermal_beam: no beam is set (cetkmc_set_beam)");
    if (u < h->ts.beam.u0 || u >= h->ts.beam.u0 + h->ts.beam.n_u)
        return fail("cetkmc_thermal_beam: update ordinal " + std::to_string(u) + " is outside the beam table's rows [" + std::to_string(h->ts.beam.u0) + ", " +
                    std::to_string(h->ts.beam.u0 + h->ts.beam.n_u) + ")");
    if (h->ts.bc_on) CHK(boundary_steps_ok("cetkmc_thermal_beam", h->ts.bc, 20 * u, 1));
    HIPCHK(hipSetDevice(h->dev));
    CHK(launch_thermal(h, dt, 1, nullptr, use_latent, scrub_nan, false, u));
    HIPCHK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the lattice shifted on the device (shift.hpp) -----------------------------------------------------
static int shift_record_ok(const std::string& f, const struct cetkmc_shift& s, const std::string& which)
{
    if (s.fill_state < 0 || s.fill_state > 4) return fail(f + ": " + which + "fill_state " + std::to_string(s.fill_state) + " is outside 0..4");
    if (s.T_mode != CETKMC_SHIFT_T_VALUE && s.T_mode != CETKMC_SHIFT_T_EDGE) return fail(f + ": " + which + "unknown T_mode " + std::to_string(s.T_mode));
    if (s.pad != 0) return fail(f + ": " + which + "pad must be 0");
    return 0;
}
static uint64_t bits_of(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }

// The lattices hs[r] moved by s[r].d and brought to the state an upload of the five new fields leaves (upload_impl), in one
// launch sequence whatever their number: a single handle passes its job by value, an ensemble a device table of jobs, and
// every kernel takes its lattice from blockIdx.y (shift.hpp).  Every array goes through a spare in its handle's scratch buffer
// and back; the spare is as large as the largest array moved.  One synchronisation and one copy of the count records.
static int shift_lattices(const std::vector<Handle*>& hs, const struct cetkmc_shift* s, struct cetkmc_shift_info* info, bool table)
{
    Handle* h0 = hs[0];
    const int L = h0->L, R = (int)hs.size();
    const int64_t n = (int64_t)L * L * L;
    std::vector<ShiftJob> jobs((size_t)R);
    int n_active = 0;
    for (int r = 0; r < R; ++r) {
        ShiftJob& J = jobs[(size_t)r];
        memset(&J, 0, sizeof J);
        for (int a = 0; a < 3; ++a) J.d[a] = std::max(-L, std::min(L, (int)s[r].d[a]));      // |d_a| >= L: everything is exposed
        J.active = J.d[0] || J.d[1] || J.d[2];
        n_active += J.active;
        if (!J.active && info) { memset(info + r, 0, sizeof *info); info[r].calls = hs[(size_t)r]->shift_calls; info[r].kept = n; }
    }
    if (!n_active) return 0;
    HIPCHK(hipSetDevice(h0->dev));
    hipStream_t st = h0->stream;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    // one block of count records (and, for an ensemble, the job table) in the scratch buffer of the first lattice; the spares
    // of every lattice in its own
    bool solid = false, origin = false, vec_maps = true, vec_g = true;
    size_t o_cnt0 = 0, o_tab0 = 0;
    for (int r = 0; r < R; ++r) {
        Handle* h = hs[(size_t)r];
        ShiftJob& J = jobs[(size_t)r];
        const Slab& sl = h->slabs[0];
        size_t words = sl.nT;
        if (h->solid_on) words = std::max(words, (size_t)3 * n);
        if (h->origin_on) words = std::max(words, std::max((size_t)n, (size_t)5 * L));
        const size_t o_st = up(words * 8), o_df = o_st + up(sl.nS), o_cnt = o_df + up(sl.nS), o_tab = o_cnt + up((size_t)R * SHIFT_NCNT * 8);
        if (J.active || r == 0) CHK(ensure_scratch(h, o_tab + (size_t)R * sizeof(ShiftJob)));
        if (r == 0) { o_cnt0 = o_cnt; o_tab0 = o_tab; }
        if (!J.active) continue;
        char* sp = (char*)h->d_scratch;
        J.S = view_of(h, 0);
        J.prev = sl.prev;
        J.arr[SHIFT_THETA] = (unsigned long long*)sl.v.theta; J.arr[SHIFT_PHI] = (unsigned long long*)sl.v.phi;
        J.arr[SHIFT_T] = (unsigned long long*)sl.Tbuf[h->cur];
        J.fill[SHIFT_THETA] = bits_of(s[r].fill_theta); J.fill[SHIFT_PHI] = bits_of(s[r].fill_phi); J.fill[SHIFT_T] = bits_of(s[r].fill_T);
        J.sp_w = (unsigned long long*)sp; J.sp_st = (uint8_t*)(sp + o_st); J.sp_df = (uint8_t*)(sp + o_df);
        J.fill_state = (int)s[r].fill_state; J.edge = s[r].T_mode == CETKMC_SHIFT_T_EDGE;
        if (h->solid_on) {
            solid = true;
            J.arr[SHIFT_STAMP] = (unsigned long long*)h->solid.stamp; J.arr[SHIFT_TS] = (unsigned long long*)h->solid.Ts;
            J.arr[SHIFT_G] = (unsigned long long*)h->solid.g; J.arr[SHIFT_COOL] = (unsigned long long*)h->solid.cool;
            J.snap = h->solid.snap; J.Tsnap = h->solid.Tsnap;
        }
        if (h->origin_on) {
            origin = true;
            J.arr[SHIFT_WORDS] = h->origin.words; J.arr[SHIFT_CENSUS] = (unsigned long long*)h->origin.census;
        }
        for (int a = SHIFT_STAMP; a < SHIFT_CENSUS; ++a)
            if (J.arr[a] && ((uintptr_t)J.arr[a] & 15)) (a == SHIFT_G ? vec_g : vec_maps) = false;
    }
    char* sp0 = (char*)h0->d_scratch;           // (ensured above with room for the records and the table, also when lattice 0 rests)
    unsigned long long* d_cnt = (unsigned long long*)(sp0 + o_cnt0);
    ShiftJob* d_jobs = table ? (ShiftJob*)(sp0 + o_tab0) : nullptr;
    for (int r = 0; r < R; ++r) jobs[(size_t)r].cnt = d_cnt + (size_t)r * SHIFT_NCNT;
    HIPCHK(hipMemsetAsync(d_cnt, 0, (size_t)R * SHIFT_NCNT * 8, st));
    if (table) {
        HIPCHK(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)R * sizeof(ShiftJob), hipMemcpyHostToDevice, st));
        h0->cnt.bytes_h2d += (int64_t)R * (int64_t)sizeof(ShiftJob);
    }
    const ShiftJob J0 = jobs[0];
    const unsigned uR = (unsigned)R;

    // state and defect mask, the dropped voxels counted from the old state; prev_state and the class bytes with the copy back
    const int64_t lanes = (int64_t)L * L * ((L + 7) / 8);
    const dim3 gb((unsigned)((lanes + 255) / 256), uR);
    hipLaunchKernelGGL(k_shift_bytes, gb, dim3(256), 0, st, J0, (const ShiftJob*)d_jobs);
    hipLaunchKernelGGL(k_shift_bytes_back, gb, dim3(256), 0, st, J0, (const ShiftJob*)d_jobs);
    HIPCHK(hipGetLastError());

    // a 64-bit array of every lattice into its spare and back (the same kernel with the identity)
    auto move = [&](int a, int n0, int n1, int n2, int W, long long base, long long plane, long long row, uint64_t fill, bool vec, bool count) {
        vec = vec && !(base & 1) && !(plane & 1) && !(row & 1);
        const int64_t thr = (int64_t)n0 * n1 * ((W * n2 + 7) / 8);
        const dim3 g((unsigned)((thr + 255) / 256), uR);
        // (one lattice: its job's share as scalars; `fill` of a map array is the constant)
        unsigned long long* arr = J0.arr[a];
        const unsigned long long f1 = a <= SHIFT_T ? J0.fill[a] : (unsigned long long)fill;
        for (int back = 0; back < 2; ++back) {
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, g, dim3(256), 0, st, (const ShiftJob*)d_jobs, arr, J0.sp_w, f1, J0.d[0], J0.d[1], J0.d[2], J0.edge, J0.cnt, a, back,
                                   n0, n1, n2, W, base, plane, row, (unsigned long long)fill);
            };
            if (count && !back) go(k_shift_words<false, true>);
            else if (vec) go(k_shift_words<true, false>);
            else go(k_shift_words<false, false>);
        }
    };
    const long long f_plane = (long long)L * h0->pitchT, f_base = 2 * f_plane;      // plane i is local plane i + 2
    for (int a = SHIFT_THETA; a <= SHIFT_T; ++a) move(a, L, L, L, 1, f_base, f_plane, h0->pitchT, 0, true, false);
    HIPCHK(hipGetLastError());

    // the rest of an upload of a state and of orientations
    const int nloc = L;
    hipLaunchKernelGGL(k_shift_clear, dim3(1024, uR), dim3(256), 0, st, J0, (const ShiftJob*)d_jobs);
    hipLaunchKernelGGL(k_shift_ifc_rebuild, dim3(2048, uR), dim3(256), 0, st, J0, (const ShiftJob*)d_jobs);
    hipLaunchKernelGGL(k_shift_ifc_relist, dim3((unsigned)((nloc * L + RELIST_ROWS - 1) / RELIST_ROWS), uR), dim3(256), 0, st, J0, (const ShiftJob*)d_jobs);
    hipLaunchKernelGGL(k_shift_orient, dim3(1024, uR), dim3(256), 0, st, J0, (const ShiftJob*)d_jobs);
    HIPCHK(hipGetLastError());

    if (solid) {
        const long long LL = (long long)L * L;
        move(SHIFT_STAMP, L, L, L, 1, 0, LL, L, ~0ull, false, true);
        move(SHIFT_TS, L, L, L, 1, 0, LL, L, 0ull, vec_maps, false);
        move(SHIFT_G, L, L, L, 3, 0, 3 * LL, 3 * L, 0ull, vec_g, false);
        move(SHIFT_COOL, L, L, L, 1, 0, LL, L, 0ull, vec_maps, false);
        const dim3 gs = solid_update_grid(L, h0->pitchT, R, 256);
        hipLaunchKernelGGL(k_shift_snapshot, gs, dim3(256), 0, st, J0, (const ShiftJob*)d_jobs);
        HIPCHK(hipGetLastError());
    }
    if (origin) {
        move(SHIFT_WORDS, L, L, L, 1, 0, (long long)L * L, L, 0ull, vec_maps, false);
        move(SHIFT_CENSUS, L, 1, 1, 5, 0, 5, 5, 0ull, false, false);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_shift_finish, dim3((uR + 63) / 64), dim3(64), 0, st, J0, (const ShiftJob*)d_jobs, R);
    HIPCHK(hipGetLastError());

    std::vector<unsigned long long> c((size_t)R * SHIFT_NCNT);
    HIPCHK(hipMemcpyAsync(c.data(), d_cnt, c.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    h0->cnt.bytes_d2h += (int64_t)c.size() * 8;
    for (int r = 0; r < R; ++r) {
        const ShiftJob& J = jobs[(size_t)r];
        if (!J.active) continue;
        Handle* h = hs[(size_t)r];
        const unsigned long long* cr = c.data() + (size_t)r * SHIFT_NCNT;
        grow_ifc_grid(h, (int)cr[7]);
        ++h->state_uploads;
        ++h->shift_calls;
        if (h->solid_on) h->solid_recorded = (int64_t)cr[6];
        invalidate(h, Cause::upload_T_or_state);
        if (info) {
            int64_t kept = 1;
            for (int a = 0; a < 3; ++a) kept *= L - std::abs(J.d[a]);
            info[r].calls = h->shift_calls; info[r].kept = kept; info[r].exposed = n - kept;
            for (int x = 0; x < 6; ++x) info[r].dropped[x] = (int64_t)cr[x];
        }
    }
    return 0;
}

// the checks of the single-lattice calls, before anything is allocated or launched
static int shift_single_ok(const std::string& f, Handle* h, const struct cetkmc_shift* s)
{
    if (!h) return fail(f + ": null handle");
    if (!s) return fail(f + ": null argument s");
    CHK(shift_record_ok(f, *s, ""));
    return one_slab_only(h, f, "");
}

int cetkmc_shift(void* handle, const struct cetkmc_shift* s, struct cetkmc_shift_info* info)
{
    Handle* h = (Handle*)handle;
    CHK(shift_single_ok("cetkmc_shift", h, s));
    return shift_lattices({h}, s, info, false);
}

int cetkmc_time_shift(void* handle, const struct cetkmc_shift* s, struct cetkmc_shift_info* info, double* ms)
{
    const std::string f = "cetkmc_time_shift";
    if (!handle) return fail(f + ": null handle");
    if (!s || !ms) return fail(f + ": null argument");
    Ens* e = ens_of(handle);
    Handle* h = (Handle*)handle;
    if (e) { for (int r = 0; r < e->R; ++r) CHK(shift_record_ok(f, s[r], "replica " + std::to_string(r) + ": ")); }
    else CHK(shift_single_ok(f, h, s));
    HIPCHK(hipSetDevice(h->dev));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    CHK(e ? shift_lattices(e->reps, s, info, true) : shift_lattices({h}, s, info, false));
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    float t = 0.0f;
    HIPCHK(hipEventElapsedTime(&t, h->ev0, h->ev1));
    *ms = (double)t;
    return 0;
}

int cetkmc_ensemble_shift(void* handle, const struct cetkmc_shift* s, struct cetkmc_shift_info* info)
{
    const std::string f = "cetkmc_ensemble_shift";
    if (!handle) return fail(f + ": null handle");
    if (!s) return fail(f + ": null argument s");
    Ens* e = ens_of(handle);
    if (!e) return fail(f + ": not an ensemble handle (cetkmc_create_ensemble)");
    for (int r = 0; r < e->R; ++r) CHK(shift_record_ok(f, s[r], "replica " + std::to_string(r) + ": "));
    return shift_lattices(e->reps, s, info, true);
}

}  // extern "C"
