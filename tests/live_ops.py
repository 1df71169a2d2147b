"""Operation scripts for one LIVE handle, with their oracle twins (test-only; nothing here needs a GPU to import).

The host layer of the library caches what it derives from the lattice (rate table, interface sums and list, row sums, class
bytes, the previous state, staged inputs, grow-only work buffers) and every entry point that changes the lattice or its
parameters resets its own subset of the freshness flags.  A script is a deterministic list of operations on ONE handle and
ONE oracle.Lattice: *mutators* (each a pair: the Engine call and what is done to the oracle lattice so that both hold the same
problem), *read-only calls* (which must change nothing) and *stepping paths* (each with its oracle call).  ``Runner`` plays
a script on the oracle alone (tests/test_live_ops_host.py checks there that the scripts cover what they claim) or on the
oracle and an Engine together, comparing after every operation (tests/test_gpu_live_handle_vs_oracle.py).

Temperature updates use dt = 5e-8 s: with the model's constants the explicit update is stable only below
dx^2 / (6 alpha) = 6.1e-8 s, and at run_kmc's 1e-6 s the field degenerates to the two clip values within three updates --
no deposition candidate then keeps a finite non-zero rate and the deposition parameters stop mattering.  One direct update
of the scripts runs at 1e-6 all the same.

A second vocabulary sits beside the first (MUTATORS2, SETTINGS, READ_ONLY2, extra_paths(); scripts pairs2:*, walk2, toggles,
stopped, pairs2_deferred): direct melt passes, the timers that really update the field, the switches of remelting and of
sub-stepped updates, the local Mode B loop, and the documented refusals between them, which a script walks THROUGH (the
refused call must have changed nothing).  While a switch is on, the oracle side of a run_steps call is one persistent
tests/substep_ref.Stepper."""
import ctypes

import numpy as np

from helpers import FOUR_KIND_PARAMS, count_deferred, dep_species

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
COUNTER_SEED = 5
THERMAL_DT = 5e-8
T_MELT = 3695.0

# ---- problems --------------------------------------------------------------------------------------------------------------
def t_field(L, seed, nan=False):
    """Ramp along k that crosses the melting point in the last plane (finite, non-zero deposition rates there; nucleation
    below), a smooth ripple across i and j so that no two rows are alike; ``nan``: two non-finite voxels."""
    rs = np.random.RandomState(7000 + seed)
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    lo = 3050.0 + 100.0 * rs.random_sample()
    T = lo + (T_MELT + 0.5 - lo) * (k / (L - 1.0)) + 0.4 * np.sin(0.9 * i + rs.random_sample()) * np.cos(0.7 * j + rs.random_sample())
    # the deposition plane i = L - 1 sits just above the melting point all over: L * L candidates with rates near nu_dep
    T[L - 1] = T_MELT + 0.3 + 0.4 * np.sin(0.8 * j[0] + rs.random_sample()) * np.cos(0.6 * k[0])
    if nan:
        T[rs.randint(L), rs.randint(L), rs.randint(L - 2)] = np.nan
        T[rs.randint(L), rs.randint(L), rs.randint(L - 2)] = np.inf
    return np.ascontiguousarray(T)


def state_field(L, seed, fill=0.03):
    rs = np.random.RandomState(8000 + seed)
    state = np.zeros((L, L, L), np.int64)
    occ = rs.random_sample((L, L, L)) < fill
    state[occ] = rs.choice([1, 2, 3, 4], size=(L, L, L), p=[0.6, 0.15, 0.2, 0.05])[occ]
    return state


def orient_fields(L, seed):
    """Orientations on every site: the attachment rate reads the empty site's stored angles too."""
    rs = np.random.RandomState(9000 + seed)
    return rs.uniform(0, np.pi, (L, L, L)), rs.uniform(0, 2 * np.pi, (L, L, L))


def defect_mask(L, seed, frac=0.3):
    return (np.random.RandomState(10000 + seed).random_sample((L, L, L)) < frac).astype(np.int64)


def fields(L, seed):
    th, ph = orient_fields(L, seed)
    return state_field(L, seed), th, ph, t_field(L, seed), defect_mask(L, seed)


def frozen_fields(L, seed):
    """A lattice the oracle terminates on after three events (with FROZEN_PARAMS): the deposition plane i = L - 1 full of
    immobile state-4 voxels (no deposition candidate, nothing that diffuses or attaches), the rest empty and within
    delta_T_c of the melting point (no nucleation) except three cold voxels, each good for one nucleation."""
    rs = np.random.RandomState(11000 + seed)
    state = np.zeros((L, L, L), np.int64)
    state[L - 1] = 4
    T = np.full((L, L, L), T_MELT - 5.0)
    for q in range(3):      # one per octant parity pattern, far apart: Mode B picks them in different super-steps
        T[1 + 5 * q, 2 + rs.randint(L - 4), 2 + rs.randint(L - 4)] = 3000.0
    th, ph = orient_fields(L, seed)
    return state, th, ph, T, np.zeros((L, L, L), np.int64)


# the nucleation of a cold voxel (4.98e13) passes the threshold; the new atom's diffusion (<= 3.8e13) and, without the
# gradient term, every attachment (<= nu = 1e13) do not
FROZEN_PARAMS = dict(I0=5e13, rate_threshold=4.5e13, anisotropy=0.0)
BASE_PARAMS = dict(FOUR_KIND_PARAMS, nu_dep=2e13, delta_T_c=10.0, anisotropy=0.25, rate_threshold=1e-30, K_nuc=500.0,
                   impurity_c=IMPURITY_C)
ALT_PARAMS = dict(I0=3e11, nu_dep=0.7e13, delta_T_c=120.0, anisotropy=1.0, rate_threshold=1e9, K_nuc=300.0, impurity_c=0.3)
assert set(ALT_PARAMS) == set(BASE_PARAMS)
# The deposition rate nu_dep * exp((T - T_melt) / (kT T)) leaves the doubles 230 K above the melting point, and latent heat
# (+1515 K per new atom) gets there at once: a clip just above T_melt keeps every total finite and the event mix balanced.
FIXED_PARAMS = dict(T_clip_hi=T_MELT + 2.0)
LASER_POWER = 2.0            # W: +0.35 K per update of 5e-8 s at the spot -- the deposition rates there triple, no more

OPTION_DEFAULTS = dict(sweep_variant=1, interface_every_step=0, apply_in_sweep=1, thermal_variant=1, thermal_planes_per_block=4,
                       thermal_planes_per_block16=16, thermal_lookahead=0, thermal_table=1, reserve_batch=0, substep_block=0,
                       substep_planes=0)
OPTION_MUTATORS = ([("sweep_variant", v) for v in range(5)] + [("interface_every_step", 1), ("apply_in_sweep", 0)] +
                   [("thermal_variant", v) for v in (0, 2, 3, 4, 5)] +
                   [("thermal_planes_per_block", 3), ("thermal_planes_per_block16", 5), ("thermal_lookahead", 1),
                    ("thermal_table", 0), ("reserve_batch", 64)])
READ_ONLY = ("download", "download_planes", "row_sums", "enumerate_events", "species_counts", "gather_species", "clusters",
             "import_clusters", "front_stats", "layer_profile", "texture_profile", "grain_table", "counters_reset",
             "reset_counters", "sync")
SINGLE_SLAB_ONLY = ("clusters", "import_clusters", "front_stats", "layer_profile", "texture_profile", "grain_table")

# mutator name -> class (the unit of "the first call after a mutator of this class sees every event kind")
MUTATORS = dict(upload_full="upload", upload_T="upload", upload_T_nan="upload", upload_orient="upload", upload_state="upload",
                upload_defects="upload", set_defects="defects", set_defects_sparse="defects", set_defects_sparse_empty="defects",
                thermal_cet="thermal", thermal_cet_noscrub_1e6="thermal", thermal_laser="thermal", thermal_laser_nolatent="thermal",
                set_prev_state="prev", set_prev_state_none="prev", apply_event="apply", staged="staged")
MUTATORS.update({"param_" + k: "params" for k in BASE_PARAMS})
MUTATORS.update({f"opt_{k}={v}": "options" for k, v in OPTION_MUTATORS})
NOOP_CLASSES = ("options",)          # documented no-ops: the next sweep is identical


def stepping_paths(L):
    """name -> spec.  run_steps: rng_mode 0 / 1 / 2, incremental or not, thermal_mode 0 / 1 / 2, batches whose temperature
    update falls first (step0 % 20 == 0: offsets 0 and 20), last or inside (offset 19) or not at all (offset 1); the
    single-call loop; run_supersteps with box 8 (k_domain_pick8), box 12 (k_domain_pick; where 12 divides L) and box == L,
    with and without null events."""
    p = dict(
        a_rng0_full_cet_first=dict(kind="run", step0=0, n=6, rng_mode=0, incremental=False, thermal_mode=1),
        a_rng0_incr_laser_inside=dict(kind="run", step0=19, n=5, rng_mode=0, incremental=True, thermal_mode=2),
        a_rng1_full_laser_none=dict(kind="run", step0=1, n=7, rng_mode=1, incremental=False, thermal_mode=2),
        a_rng1_incr_cet_first20=dict(kind="run", step0=20, n=5, rng_mode=1, incremental=True, thermal_mode=1),
        a_rng1_full_cet_last=dict(kind="run", step0=19, n=2, rng_mode=1, incremental=False, thermal_mode=1),
        a_rng2_full_nothermal=dict(kind="run", step0=1, n=6, rng_mode=2, incremental=False, thermal_mode=0),
        a_rng2_incr_laser_first=dict(kind="run", step0=40, n=6, rng_mode=2, incremental=True, thermal_mode=2),
        loop_single_calls=dict(kind="loop", n=3),
        b_box8=dict(kind="super", step0=3, n=4, box=8, null_events=False, thermal_mode=1),
        b_box8_null_laser=dict(kind="super", step0=18, n=5, box=8, null_events=True, thermal_mode=2),
        b_boxL=dict(kind="super", step0=19, n=4, box=L, null_events=False, thermal_mode=1),
        b_boxL_null=dict(kind="super", step0=0, n=3, box=L, null_events=True, thermal_mode=2),
    )
    if L % 12 == 0:
        p.update(b_box12=dict(kind="super", step0=7, n=3, box=12, null_events=False, thermal_mode=2),
                 b_box12_null=dict(kind="super", step0=20, n=3, box=12, null_events=True, thermal_mode=1))
    return p


def deferred_paths():
    """L > 128: the default path defers (cetkmc_counters.deferred_steps proves it); the same with apply_in_sweep off."""
    return dict(a_deferred=dict(kind="run", step0=17, n=4, rng_mode=1, incremental=False, thermal_mode=2),
                a_deferred_off=dict(kind="run", step0=38, n=3, rng_mode=1, incremental=False, thermal_mode=2, apply_in_sweep=0))


# ---- the second vocabulary: remelting, sub-stepped updates, the local Mode B loop, the timers ---------------------------------
# It sits BESIDE the first.  MUTATORS, READ_ONLY and stepping_paths() feed the seeded scripts pairs / walk / modes / frozen /
# pairs_deferred, whose seeds were chosen so that no pick hangs on the last bits of a total: tests/test_live_ops_host.py pins
# those scripts by hash, and nothing below may be added to the three of them.
# set_remelt_on takes melt_threshold() of the lattice as it stands (the hottest eighth of the occupied voxels melts at the next
# update, and whatever is deposited in the hot plane i = L - 1 afterwards at the one after); where there is none, this one
REMELT_ON_THRESHOLD = T_MELT + 0.3
TIMED_DT = 1e-6                        # the dt of cetkmc_time_thermal (include/cetkmc.h)
TIMED_UPDATES = 2
TIMED_PASSES = 2                       # cetkmc_time_remelt(n): n timed passes and one untimed cetkmc_remelt
SETTINGS = ("set_remelt_on", "set_remelt_off", "set_substeps=3", "set_substeps=5", "set_substeps=1")
OPTION_MUTATORS2 = [("substep_block", v) for v in (0, 1, 3)] + [("substep_planes", v) for v in (0, 8)]
MUTATORS2 = {s: "setting" for s in SETTINGS}     # (first: what the stepping loop melts has the rest of a pairs2 script to refill)
MUTATORS2.update(remelt="remelt", time_remelt="remelt", remelt_nothing="remelt_noop", time_thermal_cet="timed_thermal",
                 time_thermal_laser="timed_thermal")
MUTATORS2.update({f"opt_{k}={v}": "options" for k, v in OPTION_MUTATORS2})
# the lattice is the same behind these: a pass with threshold +inf, a switch (it changes what LATER stepping calls do), an option
NOOP_CLASSES2 = NOOP_CLASSES + ("remelt_noop", "setting")
READ_ONLY2 = ("remelt_info", "substep_info", "time_sweeps", "event_overhead", "solid_cycle", "origin_cycle")
# the fragments of the documented refusals (include/cetkmc.h) a script may walk through
REFUSED_MELT_ON = "refused while remelting is on"
REFUSED_SUBSTEPS = "refused while thermal_substeps > 1"
REFUSED_LOOKAHEAD = "thermal_lookahead on"
REFUSED_SLABS = "needs the whole lattice in one slab"


def extra_paths():
    """The local Mode B loop twice (several events per box up to a finite horizon with the update on step0; two events per
    box without a horizon), a Mode A call from step 39 and the batch that the ``stopped`` script cuts on update step 20."""
    return dict(local_k4=dict(kind="local", step0=20, n=3, K=4, horizon=2.0, thermal_mode=1),
                local_k2_inf=dict(kind="local", step0=5, n=3, K=2, horizon=float("inf"), thermal_mode=0),
                a_rng1_full_laser_39=dict(kind="run", step0=39, n=3, rng_mode=1, incremental=False, thermal_mode=2),
                a_stop=dict(kind="run", step0=0, n=30, rng_mode=0, incremental=False, thermal_mode=2))


def paths2(L):
    """the stepping paths of the pairs2 scripts: every path of the first vocabulary and the two local ones"""
    x = extra_paths()
    return dict(stepping_paths(L), local_k4=x["local_k4"], local_k2_inf=x["local_k2_inf"])


def melt_threshold(lat):
    """The threshold of a direct pass, from the oracle lattice alone: halfway between two neighbours among the occupied
    voxels' temperatures, so that the pass melts about an eighth of them -- at least 3, at most a quarter -- and no decision
    hangs on the last bits (relative gap of both neighbours to the threshold >= 2e-9).  None where no such value exists."""
    occ = lat.state != 0
    t = lat.T[occ]
    n_occ, n_inf = len(t), int(np.isposinf(t).sum())
    t = np.sort(t[np.isfinite(t)])[::-1]
    lo, hi = max(3 - n_inf, 1), min(n_occ // 4 - n_inf, len(t) - 1)
    want = min(max(n_occ // 8 - n_inf, lo), hi)
    for m in sorted(range(lo, hi + 1), key=lambda m: abs(m - want)):
        if t[m - 1] - t[m] >= 4e-9 * abs(t[m - 1]):
            return 0.5 * (t[m - 1] + t[m])
    return None


# ---- scripts: lists of dict(kind="mut" | "ro" | "step" | "opt" | "set", name=..., seed=...) -----------------------------------------
def _mut(name, seed):
    return dict(kind="mut", name=name, seed=seed)


def _mutator_block(name, seed, path_spec, pname=None, step_seed=None):
    """The operations that make up mutator ``name`` ahead of stepping path ``path_spec`` (the staged batch names the call
    whose inputs it stages)."""
    ops = []
    if name == "staged":
        return [dict(kind="mut", name=name, seed=seed, path=pname, step_seed=step_seed)]
    if name == "set_prev_state_none":        # prev := state changes something only where they differ: make them
        ops.append(_mut("set_prev_state", seed + 500))
    if name == "set_defects_sparse_empty":   # clears something only if something is set
        ops.append(_mut("set_defects_sparse", seed + 500))
    ops.append(_mut(name, seed))
    if name == "opt_sweep_variant=0" and path_spec["kind"] == "super":       # Mode B needs a streaming variant
        ops.append(dict(kind="opt", name="opt_sweep_variant=1"))
    return ops


def _restore(name):
    """Back to the default after an option mutator's pair."""
    if not name.startswith("opt_"):
        return []
    key = name[4:].split("=")[0]
    return [dict(kind="opt", name=f"opt_{key}={OPTION_DEFAULTS[key]}")]


def _step(pname, seed, staged=False):
    return dict(kind="step", name=pname, seed=seed, staged=staged)


def pairs_script(L, pname, paths=None, seed=0):
    """For stepping path S = ``pname`` and every mutator M: a warm-up call of S (every cache fresh), M, S again -- chained on
    one handle, so the S behind one mutator is the warm-up of the next."""
    paths = paths or stepping_paths(L)
    spec = paths[pname]
    ops = [_step(pname, seed)]
    for q, name in enumerate(MUTATORS):
        s = seed + 10 * (q + 1)
        ops += _mutator_block(name, s, spec, pname, s + 1)
        ops.append(_step(pname, s + 1, staged=(name == "staged")))
        ops += _restore(name)
    return ops


def deferred_pairs_script(seed=0):
    """L > 128: every mutator once, the stepping path alternating between the deferring default and apply_in_sweep off."""
    paths = deferred_paths()
    names = list(paths)
    ops = [_step(names[0], seed), _step(names[1], seed + 1)]
    for q, name in enumerate(MUTATORS):
        pname = names[q % 2]
        s = seed + 10 * (q + 1)
        ops += _mutator_block(name, s, paths[pname], pname, s + 1)
        ops.append(_step(pname, s + 1, staged=(name == "staged")))
        ops += _restore(name)
    return ops


def walk_script(L, n_ops=200, seed=0):
    """A seeded random walk over all mutators, read-only calls and stepping paths; whatever it draws, every one of them occurs
    (two shuffled rounds of each come first), and a stepping call follows at least every third operation."""
    rs = np.random.RandomState(12000 + seed)
    paths = list(stepping_paths(L))
    pool = [("mut", m) for m in MUTATORS] + [("ro", r) for r in READ_ONLY] + [("step", p) for p in paths]
    pool += [("mut", "apply_event"), ("mut", "staged")] * 2          # the classes of one mutator: as many first calls as the others
    order = [pool[q] for q in rs.permutation(len(pool))] + [pool[q] for q in rs.permutation(len(pool))]
    while len(order) < n_ops:
        order.append(pool[rs.randint(len(pool))])
    ops, since, sv0 = [], 0, False
    spaths = stepping_paths(L)
    for q, (kind, name) in enumerate(order):
        s = seed + 1000 + 7 * q
        if kind != "step" and since >= 2:
            ops.append(_step(paths[rs.randint(len(paths))], s + 3))
            since = 0
        if kind == "step" or (kind == "mut" and name == "staged"):
            if kind == "mut":
                pname = [p for p in paths if spaths[p]["kind"] == "run" and spaths[p]["rng_mode"] != 2][rs.randint(4)]
                ops += _mutator_block(name, s, spaths[pname], pname, s + 1)
            else:
                pname = name
            ops.append(_step(pname, s + 1, staged=(kind == "mut")))
            since = 0
        elif kind == "mut":
            ops += _mutator_block(name, s, dict(kind="run"))
            since += 1
        else:
            ops.append(dict(kind="ro", name=name, seed=s))
            since += 1
    ops.append(_step(paths[0], seed + 5))
    # Mode B refuses sweep_variant 0: switch back ahead of every super-step call that would meet it
    out, sv = [], 1
    for op in ops:
        if op["name"].startswith("opt_sweep_variant="):
            sv = int(op["name"].split("=")[1])
        if op["kind"] == "step" and spaths[op["name"]]["kind"] == "super" and sv == 0:
            out.append(dict(kind="opt", name="opt_sweep_variant=1"))
            sv = 1
        out.append(op)
    return out


def modes_script(L, seed=0):
    """Mode A batch -> Mode B box 8 -> Mode A incremental -> Mode B box 12 -> Mode B box 8 again (buffers grown by the box 12
    call, D shrinks back) -> box == L -> Mode A.  Where 12 does not divide L the box 12 call is box 8 with null events."""
    big = "b_box12" if L % 12 == 0 else "b_box8_null_laser"
    chain = ["a_rng1_full_cet_last", "b_box8", "a_rng0_incr_laser_inside", big, "b_box8", "b_boxL", "a_rng1_full_laser_none",
             "b_box8_null_laser", "a_rng2_incr_laser_first", "b_boxL_null", "a_rng0_full_cet_first"]
    return [_step(p, seed + q) for q, p in enumerate(chain)]


FROZEN_UNFREEZERS = ("upload_T", "param_rate_threshold", "thermal_cet_noscrub_1e6", "upload_full")
FROZEN_STEPS = dict(frozen_a=dict(kind="run", step0=1, n=8, rng_mode=1, incremental=False, thermal_mode=0),
                    frozen_b=dict(kind="super", step0=0, n=12, box=8, null_events=False, thermal_mode=0))


def frozen_script(L, seed=0):
    """The oracle terminates (status 1) inside a Mode A batch, then inside a Mode B batch.  Each is followed by an option
    (cannot unfreeze: the next call ends at once) and by every mutator that can unfreeze; then the lattice is frozen anew."""
    ops = []
    for pname in FROZEN_STEPS:
        for q, m in enumerate(FROZEN_UNFREEZERS):
            s = seed + 100 * q
            ops += [_mut("freeze", s), dict(kind="step", name=pname, seed=s + 1, staged=False, expect="terminates"),
                    dict(kind="opt", name="opt_interface_every_step=1"),
                    dict(kind="step", name=pname, seed=s + 2, staged=False, expect="stays_frozen"),
                    dict(kind="opt", name="opt_interface_every_step=0"),
                    _mut(m, s + 3), dict(kind="step", name=pname, seed=s + 4, staged=False, expect="unfrozen")]
    return ops


def script_names(L):
    return [f"pairs:{p}" for p in stepping_paths(L)] + ["walk", "modes", "frozen"]


# ---- scripts over the second vocabulary ------------------------------------------------------------------------------------------
def _set(name):
    return dict(kind="set", name=name)


def _opt(name):
    return dict(kind="opt", name=name)


def _is_mode_b(spec):
    return spec["kind"] in ("super", "local")


# A temperature update at 1e-6 s drives the field towards its two clip values: behind one, no threshold melts >= 3 voxels and <= a
# quarter of the occupied ones.  A direct pass that follows one without a new field in between gets an upload_T in front, the way
# set_prev_state_none is prepared.  Only there: the pass behind a warm rate table is what the scripts are for.
COOLERS = ("time_thermal_cet", "time_thermal_laser", "thermal_cet_noscrub_1e6")
WARMERS = ("upload_T", "upload_T_nan", "upload_full", "staged", "freeze")


def _block2(name, seed, pname, spec):
    """New mutator or setting M = ``name`` directly ahead of a call of path S = ``pname``, that call, and what puts the handle
    back.  Where S cannot run under M (Mode B with remelting on or sub-steps): M, the refused S, the switch-off, S.  A
    sub-step option is a no-op unless updates are sub-stepped: a Mode A path meets it with n = 5."""
    b, s1, s2 = _is_mode_b(spec), _step(pname, seed + 1), _step(pname, seed + 2)
    if name in ("set_remelt_on", "set_substeps=3", "set_substeps=5"):
        off = _set("set_remelt_off" if name == "set_remelt_on" else "set_substeps=1")
        return [_set(name), s1, off] + ([s2] if b else [])
    if name == "set_remelt_off":
        return [_set("set_remelt_on"), _set(name), s1]
    if name == "set_substeps=1":
        return [_set("set_substeps=5"), _set(name), s1]
    if name.startswith("opt_"):
        back = _opt(name.split("=")[0] + "=0")
        return [_opt(name), s1, back] if b or spec["kind"] == "loop" else [_set("set_substeps=5"), _opt(name), s1, back, _set("set_substeps=1")]
    if name.startswith("time_thermal"):      # two updates at 1e-6 s leave a field near its clip values: a new one behind the pair
        return [_mut(name, seed), s1, _mut("upload_T", seed + 3)]
    return [_mut(name, seed), s1]


def _with_prep(ops):
    """puts an upload_T in front of the direct passes that stand behind a COOLERS update (see there)"""
    out, cold = [], False
    for op in ops:
        if op["name"] in ("remelt", "time_remelt") and cold:
            out.append(_mut("upload_T", op["seed"] + 4))
            cold = False
        cold = (cold or op["name"] in COOLERS) and op["name"] not in WARMERS
        out.append(op)
    return out


def pairs2_script(L, pname, seed=0):
    """For stepping path S = ``pname`` (local ones included): a warm-up call of S, then for every new mutator, setting and
    option M the block of _block2, chained on one handle."""
    spec = paths2(L)[pname]
    ops = [_step(pname, seed + 3000)]
    for q, name in enumerate(MUTATORS2):
        ops += _block2(name, seed + 3000 + 10 * (q + 1), pname, spec)
    return ops


def deferred_pairs2_script(seed=0):
    """L > 128: every new mutator, setting and option once, the stepping path alternating as in deferred_pairs_script.  With
    n = 5 and no option set the update takes the default temporally blocked dispatch: three sub-steps, then the remainder."""
    paths = deferred_paths()
    names = list(paths)
    ops = [_step(names[0], seed + 3000), _step(names[1], seed + 3001)]
    for q, name in enumerate(MUTATORS2):
        pname = names[q % 2]
        ops += _block2(name, seed + 3000 + 10 * (q + 1), pname, paths[pname])
    return ops


def _legalize(ops, spaths):
    """Walks a script with the switches it sets and inserts what a call needs ahead of it: a streaming sweep variant ahead of
    Mode B (always); the switch-off of remelting and sub-steps ahead of Mode B and of thermal_lookahead = 1, the look-ahead's
    ahead of a switch-on -- these in three cases of four: the first, fifth, ... conflict of each kind is left to meet the
    documented refusal on a warm handle."""
    out, sv, ahead, melt, n = [], 1, 0, False, 1
    met = dict(mode_b=0, lookahead=0, switch=0)
    for op in ops:
        name = op["name"]
        kind = ("mode_b" if op["kind"] == "step" and _is_mode_b(spaths[name]) and (melt or n > 1) else
                "lookahead" if name == "opt_thermal_lookahead=1" and (melt or n > 1) else
                "switch" if name in ("set_remelt_on", "set_substeps=3", "set_substeps=5") and ahead else None)
        leave = kind is not None and met[kind] % 4 == 0
        if kind is not None:
            met[kind] += 1
        mode_b = op["kind"] == "step" and _is_mode_b(spaths[name])
        if name.startswith("opt_sweep_variant="):
            sv = int(name.split("=")[1])
        if mode_b and sv == 0:
            out.append(_opt("opt_sweep_variant=1"))
            sv = 1
        if (mode_b or name == "opt_thermal_lookahead=1") and (melt or n > 1) and not leave:
            out += ([_set("set_remelt_off")] if melt else []) + ([_set("set_substeps=1")] if n > 1 else [])
            melt, n = False, 1
        if name == "opt_thermal_lookahead=1" and not (melt or n > 1):
            ahead = 1
        if name in ("set_remelt_on", "set_substeps=3", "set_substeps=5"):
            if ahead and not leave:
                out.append(_opt("opt_thermal_lookahead=0"))
                ahead = 0
            if not ahead:
                melt, n = (True, n) if name == "set_remelt_on" else (melt, int(name.split("=")[1]))
        melt, n = melt and name != "set_remelt_off", 1 if name == "set_substeps=1" else n
        out.append(op)
    return out


def walk2_script(L, n_ops=200, seed=0):
    """walk_script over both vocabularies: two shuffled rounds of every mutator, setting, option, read-only call and path, a
    stepping call at least every third drawn operation, then _legalize."""
    rs = np.random.RandomState(16000 + seed)
    spaths = paths2(L)
    paths = list(spaths)
    old = stepping_paths(L)
    pool = ([("mut", m) for m in MUTATORS] + [("set" if c == "setting" else "mut", m) for m, c in MUTATORS2.items()] +
            [("ro", r) for r in READ_ONLY + READ_ONLY2] + [("step", p) for p in paths])
    order = [pool[q] for q in rs.permutation(len(pool))] + [pool[q] for q in rs.permutation(len(pool))]
    while len(order) < n_ops:
        order.append(pool[rs.randint(len(pool))])
    ops, since = [], 0
    for q, (kind, name) in enumerate(order):
        s = seed + 5000 + 7 * q
        if kind != "step" and since >= 2:
            ops.append(_step(paths[rs.randint(len(paths))], s + 3))
            since = 0
        if kind == "step":
            ops.append(_step(name, s + 1))
            since = 0
            continue
        if name == "staged":
            pname = [p for p in old if old[p]["kind"] == "run" and old[p]["rng_mode"] != 2][rs.randint(4)]
            ops += _mutator_block(name, s, old[pname], pname, s + 1) + [_step(pname, s + 1, staged=True)]
            since = 0
            continue
        ops += (_mutator_block(name, s, dict(kind="run")) if name in MUTATORS else [dict(kind=kind, name=name, seed=s)])
        since += 1
    ops.append(_step(paths[0], seed + 5))
    return _with_prep(_legalize(ops, spaths))


def toggles_script(L, seed=0):
    """Both switches through their combinations on one handle, a Mode A call that crosses an update (step0 19, 20 or 39) behind
    every change: n = 1 and no melt; n = 5; both; the melt alone; neither, with Mode B and the local loop; n = 3, incremental."""
    chain = ["a_rng1_full_cet_last", "set_substeps=5", "a_rng1_incr_cet_first20", "set_remelt_on", "a_rng1_full_laser_39",
             "set_substeps=1", "a_rng0_incr_laser_inside", "set_remelt_off", "a_rng1_full_cet_last", "b_box8", "local_k4",
             "set_substeps=3", "a_rng0_incr_laser_inside", "a_rng1_incr_cet_first20", "set_substeps=1"]
    return [_set(x) if x.startswith("set_") else _step(x, seed + 7000 + q) for q, x in enumerate(chain)]


# one operation between a batch that ran out of its stream ON update step 20 and its continuation: the marker of the applied
# update (CETKMC_CACHE_APPLIED) survives the first group -- the continuation skips the update and the melt and consumes the
# step's plane again -- and not the second (cause rows with NEW_FIELD): there the update runs again
STOPPED_KEEP = (None, "remelt", "set_remelt_on", "set_substeps=5", "time_sweeps", "remelt_info")
STOPPED_DROP = ("time_thermal_cet", "upload_defects")


def stopped_script(L, seed=0):
    ops = []
    for q, x in enumerate(STOPPED_KEEP + STOPPED_DROP):
        s = seed + 8000 + 20 * q
        ops.append(dict(_step("a_stop", s), cut=20))
        if x is not None:
            ops.append(_set(x) if x.startswith("set_") else dict(kind="ro", name=x, seed=s) if x in READ_ONLY2 else _mut(x, s + 1))
        ops.append(dict(_step("a_stop", s), resume=20, keeps=x in STOPPED_KEEP))
        ops += [_set("set_remelt_off")] * (x == "set_remelt_on") + [_set("set_substeps=1")] * (x == "set_substeps=5")
        ops += [_mut("upload_T", s + 2)] * (x == "time_thermal_cet")
    return ops


def script_names2(L):
    return [f"pairs2:{p}" for p in paths2(L)] + ["walk2", "toggles", "stopped"]


# Seeds of the second vocabulary's scripts, where seed 0 does not meet the conditions of tests/test_live_ops_host.py on the
# oracle (a melted voxel occupied again when the script ends; no pick on the last bits of a total): (script, L) -> seed.
SCRIPT_SEEDS = {("pairs2:a_rng1_incr_cet_first20", 16): 700, ("pairs2:a_rng1_incr_cet_first20", 24): 600,
                ("pairs2:a_rng1_full_cet_last", 16): 300, ("pairs2:a_rng1_full_cet_last", 24): 300,
                ("toggles", 16): 100, ("toggles", 24): 100, ("walk2", 24): 100}


def make_script(L, name):
    seed = SCRIPT_SEEDS.get((name, L))
    if seed is not None and name.startswith("pairs2:"):
        return _with_prep(pairs2_script(L, name[7:], seed=seed))
    if seed is not None:
        return dict(toggles=toggles_script, stopped=stopped_script, walk2=walk2_script)[name](L, seed=seed)
    if name.startswith("pairs:"):
        return pairs_script(L, name[6:])
    if name.startswith("pairs2:"):
        return _with_prep(pairs2_script(L, name[7:]))
    if name == "pairs_deferred":
        return deferred_pairs_script()
    if name == "pairs2_deferred":
        return _with_prep(deferred_pairs2_script())
    return dict(walk=walk_script, modes=modes_script, frozen=frozen_script, walk2=walk2_script, toggles=toggles_script,
                stopped=stopped_script)[name](L)


def tags(script, label):
    """One tag per operation: index, name and the three operations before it -- a failure names where the handle went wrong."""
    names = [op["name"] for op in script]
    return [f"{label}[{q}] {n} (after {' > '.join(names[max(0, q - 3):q]) or 'creation'})" for q, n in enumerate(names)]


# ---- the oracle side of a stepping call ------------------------------------------------------------------------------------------
def updates_before(step0, x):
    """temperature-update steps among the x global steps from step0: the source planes a stopped batch consumed before its
    stopping step"""
    return sum(1 for g in range(step0, step0 + x) if g % 20 == 0)


def clone(o, lat):
    c = o.Lattice(lat.state, lat.theta, lat.phi, lat.T, lat.defects)
    c.prev_state = lat.prev_state.copy()
    ctypes.memmove(ctypes.byref(c.params), ctypes.byref(lat.params), ctypes.sizeof(lat.params))
    c.nuc_count = lat.nuc_count
    return c


def step_inputs(L, spec, seed):
    """The host inputs of a stepping call, from its seed alone."""
    from cetkmc import synthetic
    rs = np.random.RandomState(13000 + seed)
    n = spec["n"]
    d = dict(u_pick=rs.random_sample(n), u_def=rs.random_sample(n))
    if spec["kind"] == "run":
        d["u_np"] = rs.random_sample(n * (L * L + 2) if spec["rng_mode"] == 0 else 2 * n + 2)
    else:
        d["u_np"] = rs.random_sample(2 * n)
    tm = spec.get("thermal_mode", 0)
    d["q"] = synthetic.laser_planes(L, spec["step0"], n, power=LASER_POWER) if tm == 2 and spec["kind"] != "loop" else None
    return d


def oracle_loop_event(lat, u_pick, u_def, u_np, x, scale=1.0):
    """One iteration of the single-call loop on the oracle: sweep, pick, species, orientation, defect draw.  Returns (event or
    None, r, theta, phi, make_defect, sweep)."""
    sw = lat.sweep()
    if sw["n_events"] == 0 or not (sw["total"] >= 1e-25) or not np.isfinite(sw["total"]):
        return None, 0.0, 0.0, 0.0, False, sw
    r = u_pick[x] * scale * sw["total"]
    ev = lat.select_tree(sw["blocksum"], sw["blockcnt"], sw["rowsum"], sw["rowcnt"], r)
    if ev.type == 0:
        ev.atom = dep_species(u_np[2 * x], lat.params.impurity_c, lat.params.impurity_re)
    th, ph = (u_np[2 * x] * np.pi, u_np[2 * x + 1] * 2 * np.pi) if ev.type in (0, 2) else (0.0, 0.0)
    return ev, r, th, ph, bool(u_def[x] < DEFECT_FRACTION), sw


def oracle_step(lat, spec, inp, scale=1.0):
    """The stepping call ``spec`` on the oracle lattice; ``scale`` multiplies the host stream's pick uniforms (the
    robustness probe of the host test).  The single-call loop returns dict(done, status, events) like the batched calls."""
    if spec["kind"] == "run" and spec["rng_mode"] == 2:
        # every uniform counter based: the oracle's statement of it is the single-domain super-step (include/cetkmc.h)
        r = lat.run_supersteps(spec["step0"], spec["n"], lat.L, DEFECT_FRACTION, COUNTER_SEED, thermal_mode=spec["thermal_mode"],
                               thermal_dt=THERMAL_DT, q_planes=inp["q"])
        return dict(done=r["done"], status=r["status"], q_used=r["q_used"], totals=r["totals"],
                    events=np.ascontiguousarray(r["events"][:, 0]))
    if spec["kind"] == "run":
        return lat.run_steps(spec["step0"], spec["n"], DEFECT_FRACTION, inp["u_pick"] * scale, inp["u_def"], inp["u_np"],
                             rng_mode=spec["rng_mode"], seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT,
                             q_planes=inp["q"])
    if spec["kind"] == "super":
        return lat.run_supersteps(spec["step0"], spec["n"], spec["box"], DEFECT_FRACTION, COUNTER_SEED,
                                  thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT, q_planes=inp["q"],
                                  null_events=spec["null_events"])
    evs = []
    for x in range(spec["n"]):
        ev, _, th, ph, mk, _ = oracle_loop_event(lat, inp["u_pick"], inp["u_def"], inp["u_np"], x, scale)
        if ev is None:
            return dict(done=x, status=1, events=evs)
        evs.append((ev.type, tuple(ev.pos), tuple(ev.target), ev.atom))
        lat.apply(ev, th, ph, mk)
    return dict(done=spec["n"], status=0, events=evs)


def event_kinds(spec, ro):
    """Executed events of a stepping call by kind (dep, diff, nuc, att), from the oracle's result."""
    if spec["kind"] == "loop":
        t = np.array([e[0] for e in ro["events"]], np.int64)
    else:
        t = np.asarray(ro["events"]["type"][:ro["done"]]).ravel()
    return np.bincount(t[t >= 0], minlength=4)[:4]


def event_key(spec, ro):
    if spec["kind"] == "loop":
        return repr(ro["events"])
    ev = ro["events"][:ro["done"]]
    return b"".join(np.ascontiguousarray(ev[f]).tobytes() for f in ("type", "pos", "target", "atom"))


def sweep_signature(lat):
    sw = lat.sweep()
    return (sw["total"], sw["n_events"], sw["n_dep"], sw["rowsum"].tobytes(), sw["rowcnt"].tobytes())


def mutator_signature(o, lat, cls):
    """What a mutator of class ``cls`` must change (and a no-op must not): the next sweep; for the direct temperature updates
    the field as well; for the previous state the field after the next laser update (its only reader)."""
    if cls == "impurity":        # read by no rate: the species a deposition writes (dep_species) is all it changes
        return (lat.params.impurity_c,)
    if cls == "prev":
        c = clone(o, lat)
        c.thermal_laser(THERMAL_DT, np.zeros((lat.L, lat.L)), scrub_nan=True)
        return c.T.tobytes()
    sig = sweep_signature(lat)
    return sig + (lat.T.tobytes(),) if cls in ("thermal", "timed_thermal") else sig


# ---- the runner ------------------------------------------------------------------------------------------------------------------
class Runner:
    """Plays a script on an oracle lattice and, with ``engine``, on a live handle, comparing after every operation.
    ``check_fields(engine, lat, tag)``, ``check_run(engine, lat, rg, ro, tag)`` and ``check_super(...)`` are the comparisons of
    tests/helpers.py with the tolerance bound in; ``on_step(op, spec, inp, ro, before)`` is the host test's probe."""

    def __init__(self, o, L, paths=None, engine=None, n_slabs=1, check_fields=None, check_run=None, check_super=None, seed=0,
                 check_local=None):
        self.o, self.L, self.e, self.n_slabs = o, int(L), engine, n_slabs
        self.paths = dict(stepping_paths(L), **FROZEN_STEPS, **extra_paths(), **(paths or {}))
        self.check_fields, self.check_run, self.check_super, self.check_local = check_fields, check_run, check_super, check_local
        # the second vocabulary: the two switches, the counters they feed and what the host conditions read afterwards
        self.remelt_on, self.remelt_threshold, self.substeps = False, REMELT_ON_THRESHOLD, 1
        self.info = dict(passes=0, n_melted=0, n_melted_last=0)      # cetkmc_remelt_info as it must read
        self.sub = dict(updates=0, substeps=0)                        # cetkmc_substep_info likewise
        self.last_q = np.zeros((self.L, self.L))                      # the plane of the handle's last cetkmc_thermal_laser
        self.ever_melted = np.zeros((self.L,) * 3, bool)
        self.min_gap = np.inf                 # smallest |T - threshold| / threshold over the occupied voxels at a melt decision
        self.stepper = None                   # substep_ref.Stepper, made at its first use and kept: it carries applied_g
        self.refusals = []                    # (tag, fragment) of the refused calls met
        self.last = {}                        # the last operation, for the host conditions
        self.values = dict(BASE_PARAMS)
        self.opt = dict(OPTION_DEFAULTS)
        self.opt_defaults = dict(OPTION_DEFAULTS)
        self.sweep_auto = True                # sweep_variant never set: L <= 128 runs the one-launch sweep, which does not defer
        self.deferred_expected = 0
        self.deferred_reset = 0               # deferred_steps that counters(reset=True) took away
        self.staged = False
        self.tag = "creation"
        f = fields(L, seed)
        self.lat = o.Lattice(*f, impurity_c=IMPURITY_C)
        self._push_params()
        if engine is not None:
            engine.upload(*f)
            self._verify()

    # -- both sides ------------------------------------------------------------------------
    def _push_params(self):
        both = dict(self.values, **FIXED_PARAMS)
        for k, v in both.items():
            setattr(self.lat.params, k, v)
        if self.e is not None:
            for k, v in both.items():
                setattr(self.e.params, k, v)
            self.e.set_params()

    def _verify(self):
        if self.e is not None:
            self.check_fields(self.e, self.lat, self.tag)
            assert self.e.nucleation_count() == self.lat.nuc_count, (self.tag, "nucleation_count", self.e.nucleation_count(), self.lat.nuc_count)

    def _defers(self, spec):
        o = self.opt
        return (o["apply_in_sweep"] and not spec["incremental"] and o["sweep_variant"] == 1 and not o["interface_every_step"] and
                self.n_slabs == 1 and not (self.sweep_auto and self.L <= 128) and self.L <= 256)

    def _verify_info(self):
        """cetkmc_remelt_info and cetkmc_substep_info as last read: behind every stepping call and every direct pass"""
        if self.e is not None:
            got = self.e.remelt_info()
            assert {k: got[k] for k in self.info} == self.info, (self.tag, "remelt_info", got, self.info)
            got = self.e.substep_info()
            assert {k: got[k] for k in self.sub} == self.sub, (self.tag, "substep_info", got, self.sub)

    def _refused(self, call, fragment):
        """a call the library must refuse with the documented message; what it left behind is verified by the caller"""
        self.refusals.append((self.tag, fragment))
        if self.e is None:
            return
        try:
            call()
        except RuntimeError as ex:
            assert fragment in str(ex), (self.tag, "refused with another message", str(ex), fragment)
        else:
            raise AssertionError(f"{self.tag}: the call was not refused ({fragment})")

    def _drop_marker(self):
        """a new field (upload, direct temperature update): the update a stopped batch applied is no longer remembered"""
        if self.stepper is not None:
            self.stepper.applied_g = -1

    def _note_gap(self, threshold):
        occ = self.lat.state != 0
        if np.isfinite(threshold) and occ.any():
            gap = np.abs(self.lat.T[occ] - threshold) / abs(threshold)
            gap = gap[np.isfinite(gap)]
            if len(gap):
                self.min_gap = min(self.min_gap, float(gap.min()))

    def _melt(self, threshold):
        """one pass on the oracle lattice"""
        import remelt_ref
        self._note_gap(threshold)
        occ = self.lat.state != 0
        k = remelt_ref.remelt(self.lat, threshold)
        self.ever_melted |= occ & (self.lat.state == 0)
        return k, int(occ.sum())

    def _update(self, laser, dt, q=None, latent=True, scrub=True):
        """one temperature update of the oracle lattice as the handle performs it: thermal_substeps applications"""
        import substep_ref
        lat, n = self.lat, self.substeps
        self._drop_marker()
        if n > 1:
            self.sub["updates"] += 1
            self.sub["substeps"] += n
        if n > 1 and (latent or not laser):
            substep_ref.update(lat, n, dt, 2 if laser else 1, q, use_latent=True, scrub=scrub)
            return
        dt_s = dt / n if n > 1 else dt
        for s in range(n):
            if not laser:
                lat.thermal_cet(dt=dt_s, scrub_nan=scrub)
            elif latent:
                lat.thermal_laser(dt_s, q, scrub_nan=scrub, update_prev=True)
            else:       # no latent term and the previous state stays: the oracle's term vanishes where prev == cur
                lat.thermal_laser(dt_s, q, prev_state=lat.state, scrub_nan=bool(scrub and s == 0), update_prev=False)

    def setting(self, name):
        """a switch: what later stepping calls do changes, the lattice does not"""
        e = self.e
        if name.startswith("set_remelt"):
            on = name.endswith("_on")
            thr = (melt_threshold(self.lat) or REMELT_ON_THRESHOLD) if on else REMELT_ON_THRESHOLD
            call = lambda: e.set_remelt(on, thr)
            if self.n_slabs > 1:
                return self._refused(call, REFUSED_SLABS)
            if on and self.opt["thermal_lookahead"]:
                return self._refused(call, REFUSED_LOOKAHEAD)
            self.remelt_on, self.remelt_threshold = on, thr
        else:
            n = int(name.split("=")[1])
            call = lambda: e.set_thermal_substeps(n)
            if n > 1 and self.opt["thermal_lookahead"]:
                return self._refused(call, REFUSED_LOOKAHEAD)
            self.substeps = n
        if e is not None:
            call()

    def set_option(self, key, value):
        if key == "thermal_lookahead" and value and (self.remelt_on or self.substeps > 1):
            return self._refused(lambda: self.e.set_option(key, value), REFUSED_MELT_ON if self.remelt_on else REFUSED_SUBSTEPS)
        self.opt[key] = value
        if key == "sweep_variant":
            self.sweep_auto = False
        if key == "reserve_batch":
            self.staged = False               # the library drops a staged batch when it may move the buffers
        if self.e is not None:
            self.e.set_option(key, value)

    # -- one operation -----------------------------------------------------------------------
    def do(self, op, tag=""):
        self.tag = tag or op["name"]
        try:
            return self._do(op)
        except (AssertionError, RuntimeError) as ex:      # (a call the library refused unasked: its message carries no tag)
            # where the handle stood: what the tag's three operations do not say
            alt = {k: v for k, v in self.values.items() if v != BASE_PARAMS.get(k)}
            opt = {k: v for k, v in self.opt.items() if v != self.opt_defaults[k]}
            what = f"{self.tag}: {ex}" if isinstance(ex, RuntimeError) else f"{ex}"
            raise AssertionError(f"{what}\nhandle: parameters off their base {alt}, options off their default {opt}, "
                                 f"sweep_variant {'never set' if self.sweep_auto else 'set'}, slabs {self.n_slabs}") from ex

    def _do(self, op):
        kind, name = op["kind"], op["name"]
        self.last = {}
        if kind == "step":
            return self.step(op)
        if kind == "set":
            self.setting(name)
        elif kind == "opt" or name.startswith("opt_"):
            key, value = name[4:].split("=")
            self.set_option(key, int(value))
        elif kind == "ro":
            self.read_only(name, op["seed"])
        else:
            getattr(self, "m_" + (name[:6] if name.startswith("param_") else name))(op)
        self._verify()
        return None

    # -- mutators ------------------------------------------------------------------------------
    def _new_lattice(self, f):
        old = self.lat
        self.lat = self.o.Lattice(*f)
        ctypes.memmove(ctypes.byref(self.lat.params), ctypes.byref(old.params), ctypes.sizeof(old.params))
        self.lat.nuc_count = old.nuc_count            # the count belongs to the handle: an upload leaves it (include/cetkmc.h)
        self._drop_marker()
        if self.e is not None:
            self.e.upload(*f)

    def m_upload_full(self, op):
        self._new_lattice(fields(self.L, op["seed"]))

    def m_freeze(self, op):
        self.values.update(BASE_PARAMS)
        self.values.update(FROZEN_PARAMS)
        self._push_params()
        self._new_lattice(frozen_fields(self.L, op["seed"]))

    def m_upload_T(self, op, nan=False):
        T = t_field(self.L, op["seed"], nan=nan)
        self.lat.T = T.copy()
        self._drop_marker()
        if self.e is not None:
            self.e.upload(T=T)

    def m_upload_T_nan(self, op):
        self.m_upload_T(op, nan=True)

    def m_upload_orient(self, op):
        th, ph = orient_fields(self.L, op["seed"])
        self.lat.theta, self.lat.phi = th.copy(), ph.copy()
        self._drop_marker()
        if self.e is not None:
            self.e.upload(theta=th, phi=ph)

    def m_upload_state(self, op):
        st = state_field(self.L, op["seed"])
        self.lat.state = st.astype(np.int8)
        self.lat.prev_state = self.lat.state.copy()       # cetkmc_upload: prev_state becomes the state
        self._drop_marker()
        if self.e is not None:
            self.e.upload(state=st)

    def m_upload_defects(self, op):
        m = defect_mask(self.L, op["seed"])
        self.lat.defects = m.astype(np.int8)
        self._drop_marker()                               # a defects-only upload included (cetkmc_run_args.q_planes)
        if self.e is not None:
            self.e.upload(defects=m)

    def m_set_defects(self, op):
        m = defect_mask(self.L, op["seed"], 0.5)
        self.lat.defects = m.astype(np.int8)
        if self.e is not None:
            self.e.set_defects(m)

    def m_set_defects_sparse(self, op, empty=False):
        n = self.L ** 3
        idx = np.zeros(0, np.int64) if empty else np.random.RandomState(14000 + op["seed"]).permutation(n)[:n // 5].astype(np.int64)
        m = np.zeros(n, np.int8)
        m[idx] = 1
        self.lat.defects = m.reshape((self.L,) * 3)
        if self.e is not None:
            self.e.set_defects_sparse(idx)

    def m_set_defects_sparse_empty(self, op):
        self.m_set_defects_sparse(op, empty=True)

    def m_param_(self, op):
        k = op["name"][6:]
        self.values[k] = ALT_PARAMS[k] if self.values[k] != ALT_PARAMS[k] else BASE_PARAMS[k]
        self._push_params()

    def m_thermal_cet(self, op, dt=THERMAL_DT, scrub=True):
        self._update(False, dt, scrub=scrub)
        if self.e is not None:
            self.e.thermal_cet(dt, scrub_nan=scrub)

    def m_thermal_cet_noscrub_1e6(self, op):
        self.m_thermal_cet(op, dt=1e-6, scrub=False)

    def m_thermal_laser(self, op, latent=True):
        from cetkmc import synthetic
        q = synthetic.laser_planes(self.L, 20 * (op["seed"] % 7), 1, power=4 * LASER_POWER)[0]
        self.last_q = np.array(q, np.float64)
        self._update(True, THERMAL_DT, q, latent=latent, scrub=True)
        if self.e is not None:
            self.e.thermal_laser(THERMAL_DT, q, use_latent=latent, scrub_nan=True)

    def m_thermal_laser_nolatent(self, op):
        self.m_thermal_laser(op, latent=False)

    def m_set_prev_state(self, op):
        prev = state_field(self.L, op["seed"], fill=0.01)
        self.lat.prev_state = prev.astype(np.int8)
        if self.e is not None:
            self.e.set_prev_state(prev)

    def m_set_prev_state_none(self, op):
        self.lat.prev_state = self.lat.state.copy()
        if self.e is not None:
            self.e.set_prev_state(None)

    def m_apply_event(self, op):
        rs = np.random.RandomState(15000 + op["seed"])
        u_pick, u_def, u_np = rs.random_sample(1), np.zeros(1), rs.random_sample(2)       # u_def 0: the event makes a defect
        self._loop_event(u_pick, u_def, u_np, 0)

    def m_staged(self, op):
        """cetkmc_stage_inputs for the stepping call that follows, then three mutators before that call.  A run_steps call on
        host streams consumes the staged batch (it must then step the MUTATED lattice); any other call drops it."""
        spec = self.paths[op["path"]]
        consumes = spec["kind"] == "run" and spec["rng_mode"] != 2
        if not consumes:
            spec = self.paths["a_rng1_full_laser_none"]
        inp = step_inputs(self.L, spec, op["step_seed"])
        if self.e is not None:
            self.e.stage_inputs(spec["step0"], spec["n"], DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"],
                                rng_mode=spec["rng_mode"], seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT,
                                q_planes=inp["q"], incremental=spec["incremental"])
        self.m_upload_T(dict(seed=op["seed"] + 1))
        self.m_param_(dict(name="param_I0"))
        self.m_set_defects(dict(seed=op["seed"] + 2))
        self.staged = consumes

    def m_remelt(self, op, timed=False, threshold=None):
        """cetkmc_remelt: one direct pass (cause "apply").  cetkmc_time_remelt: its twin is ONE pass, the rule being idempotent on
        an unchanged field; the counters see TIMED_PASSES timed passes and the untimed one behind them, which melts nothing."""
        e = self.e
        if self.n_slabs > 1:
            return self._refused(lambda: e.time_remelt(TIMED_PASSES, T_MELT) if timed else e.remelt(T_MELT), REFUSED_SLABS)
        thr = melt_threshold(self.lat) if threshold is None else threshold
        assert thr is not None, (self.tag, "no threshold melts >= 3 voxels and <= a quarter of the occupied ones: REMELT_PREP")
        k, occupied = self._melt(thr)
        self.last = dict(melted=k, occupied=occupied, threshold=thr)
        self.info["passes"] += 1 + TIMED_PASSES * timed
        self.info["n_melted"] += k
        self.info["n_melted_last"] = 0 if timed else k
        if e is not None:
            if timed:
                e.time_remelt(TIMED_PASSES, thr)
            else:
                got = e.remelt(thr)
                assert {x: got[x] for x in self.info} == self.info, (self.tag, "cetkmc_remelt's own info", got, self.info)
            self._verify_info()

    def m_time_remelt(self, op):
        self.m_remelt(op, timed=True)

    def m_remelt_nothing(self, op):
        """threshold +inf: no finite temperature is at or above it (an occupied +inf voxel would melt; the host test asserts that the
        scripts meet none).  The lattice stays; the pass is counted and raises its cause all the same."""
        self.m_remelt(op, threshold=np.inf)

    def m_time_thermal(self, laser):
        """cetkmc_time_thermal: TIMED_UPDATES real updates at 1e-6 s with the scrub; laser: the latent-heat term and the plane
        of the handle's last cetkmc_thermal_laser (zeros before the first)"""
        for _ in range(TIMED_UPDATES):
            self._update(laser, TIMED_DT, self.last_q if laser else None, latent=True, scrub=True)
        if self.e is not None:
            self.e.time_thermal(TIMED_UPDATES, laser=laser)
            self._verify_info()

    def m_time_thermal_cet(self, op):
        self.m_time_thermal(False)

    def m_time_thermal_laser(self, op):
        self.m_time_thermal(True)

    # -- read-only calls -------------------------------------------------------------------------
    def read_only2(self, name):
        e = self.e
        if name == "origin_cycle" and self.remelt_on:           # cetkmc_origin_begin is refused while remelting is on
            return self._refused(e.origin_begin if e is not None else None, REFUSED_MELT_ON)
        if e is None:
            return
        if name in ("remelt_info", "substep_info"):
            return self._verify_info()
        if name == "time_sweeps":
            return e.time_sweeps(3)
        if name == "event_overhead":
            return e.event_overhead(5)
        begin, body, end = ((e.solid_begin, lambda: (e.solid_update(1, THERMAL_DT), e.solid_read()), e.solid_end) if name == "solid_cycle"
                            else (e.origin_begin, e.origin_read, e.origin_end))
        try:
            begin()
            try:
                body()
            finally:
                end()
        except RuntimeError:
            if self.n_slabs == 1:                    # refused on a multi-slab handle: must change nothing either
                raise

    def read_only(self, name, seed):
        e, L = self.e, self.L
        if name in READ_ONLY2:
            return self.read_only2(name)
        if name == "reset_counters":
            self.lat.nuc_count = 0                    # cetkmc_reset_counters zeroes the step state (include/cetkmc.h)
        if e is None:
            return
        if name == "counters_reset":
            self.deferred_reset += e.counters(reset=True)["deferred_steps"]
            assert e.counters()["deferred_steps"] == 0, self.tag
            return
        calls = dict(download=lambda: e.download(defects=True), download_planes=lambda: e.download_planes(0, L, True, True, True, True, True),
                     row_sums=lambda: (e.rate_sweep(), e.row_sums()), enumerate_events=e.enumerate_events,
                     species_counts=e.species_counts, gather_species=lambda: e.gather_species(1 + seed % 4),
                     clusters=lambda: e.clusters(labels=True), import_clusters=lambda: e.import_clusters(e.clusters(labels=True)["labels"]),
                     front_stats=e.front_stats, layer_profile=e.layer_profile, texture_profile=lambda: e.texture_profile(n_bins=8),
                     grain_table=e.grain_table, reset_counters=e.reset_counters, sync=e.sync)
        try:
            calls[name]()
        except RuntimeError:
            if not (self.n_slabs > 1 and name in SINGLE_SLAB_ONLY):       # refused on a multi-slab handle: must change nothing either
                raise

    # -- stepping ----------------------------------------------------------------------------------
    def _loop_event(self, u_pick, u_def, u_np, x):
        ev, r, th, ph, mk, sw = oracle_loop_event(self.lat, u_pick, u_def, u_np, x)
        if self.e is not None:
            total, n_events, n_dep = self.e.rate_sweep()
            assert (n_events, n_dep) == (sw["n_events"], sw["n_dep"]), (self.tag, "sweep counts", n_events, n_dep, sw["n_events"], sw["n_dep"])
        if ev is None:
            return None
        if self.e is not None:
            g = self.e.select(r)
            got = (g.type, tuple(g.pos), tuple(g.target), g.dep_rank)
            assert got == (ev.type, tuple(ev.pos), tuple(ev.target), ev.dep_rank), (self.tag, "select", got, ev.astuple())
            g.atom = ev.atom
            self.e.apply(g, th, ph, mk)
        self.lat.apply(ev, th, ph, mk)
        return ev

    def _step_refusal(self, spec):
        """the fragment of the refusal a stepping call must meet on the handle as it stands (the library's order), or None"""
        if _is_mode_b(spec):
            if self.remelt_on:
                return REFUSED_MELT_ON
            if self.substeps > 1:
                return REFUSED_SUBSTEPS
            if spec["kind"] == "local" and self.n_slabs > 1:
                return REFUSED_SLABS
        return None

    def _needs_stepper(self, op):
        """With n = 1 and remelting off the oracle side of a run_steps call stays oracle.Lattice.run_steps; a switch that is
        on, a stream cut on an update step and the marker such a cut left need the composed loop."""
        return (self.remelt_on or self.substeps > 1 or "cut" in op or "resume" in op or
                (self.stepper is not None and self.stepper.applied_g >= 0))

    def _stepper_run(self, op, spec, inp):
        """the run_steps call on the ONE persistent substep_ref.Stepper of this handle, its n and threshold following the
        switches; returns the oracle's result and the inputs as the engine must get them (cut or continued streams)"""
        import substep_ref
        runner = self

        class Stepper(substep_ref.Stepper):
            def melt(self, g):
                runner._note_gap(self.threshold)
                occ = self.lat.state != 0
                k = super().melt(g)
                runner.ever_melted |= occ & (self.lat.state == 0)
                runner.last["melted"] = runner.last.get("melted", 0) + k
                return k

        if self.stepper is None:
            self.stepper = Stepper(self.lat, 1, None)
            self.stepper.info = self.info                 # one set of counters for direct passes and the loop's
        st = self.stepper
        st.lat, st.n, st.threshold = self.lat, self.substeps, self.remelt_threshold if self.remelt_on else None
        step0, n = spec["step0"], spec["n"]
        if "cut" in op:          # the stream ends where step op["cut"] would begin to read it: a probe on a clone finds the place
            x = op["cut"] - step0

            def probe(m, u_np):
                p = substep_ref.Stepper(clone(self.o, self.lat), st.n, st.threshold)
                return p.run_steps(step0, m, DEFECT_FRACTION, inp["u_pick"][:m], inp["u_def"][:m], u_np, rng_mode=spec["rng_mode"],
                                   seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT, q_planes=inp["q"])

            # (as tests/test_gpu_remelt_stepping.py builds it: what the first x steps consume; a step asks for more than it
            # consumes, so the shortest stream that still lets step x - 1 run lies at or behind that place)
            lo_ = probe(x, inp["u_np"])["np_used"]
            hi_ = min(lo_ + self.L * self.L + 2, len(inp["u_np"]))       # what one step can ask for at the most
            while lo_ < hi_:
                mid = (lo_ + hi_) // 2
                lo_, hi_ = (lo_, mid) if probe(x, inp["u_np"][:mid])["done"] >= x else (mid + 1, hi_)
            cut = self.cut = lo_
            inp = dict(inp, u_np=inp["u_np"][:cut])
        elif "resume" in op:
            x = op["resume"] - step0
            q = inp["q"]
            inp = dict(u_pick=inp["u_pick"][x:], u_def=inp["u_def"][x:], u_np=inp["u_np"][self.cut:],
                       q=None if q is None else q[updates_before(step0, x):])
            step0, n = step0 + x, n - x
        self.last.update(substeps=st.n, threshold=st.threshold, marker=st.applied_g, melted=0, inp=inp, args=(step0, n))
        before = dict(st.stats)
        ro = st.run_steps(step0, n, DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"], rng_mode=spec["rng_mode"],
                          seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT, q_planes=inp["q"])
        if st.n > 1:
            for k in self.sub:
                self.sub[k] += st.stats[k] - before[k]
        return ro, inp

    def _inputs(self, spec, op):
        """the host inputs of the stepping call ``op`` (a subclass may withhold the planes)"""
        return step_inputs(self.L, spec, op["seed"])

    def _engine_call(self, spec, inp):
        """the engine's call of a stepping path, for the refusals: nothing of its result is read"""
        e = self.e
        if spec["kind"] == "local":
            return lambda: e.run_supersteps_local(spec["step0"], spec["n"], DEFECT_FRACTION, COUNTER_SEED, spec["K"], spec["horizon"],
                                                  thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT)
        if spec["kind"] == "super":
            return lambda: e.run_supersteps(spec["step0"], spec["n"], spec["box"], DEFECT_FRACTION, COUNTER_SEED,
                                            thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT, q_planes=inp["q"],
                                            null_events=spec["null_events"])
        return lambda: e.run_steps(spec["step0"], spec["n"], DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"],
                                   rng_mode=spec["rng_mode"], seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT,
                                   q_planes=inp["q"], incremental=spec["incremental"])

    def step(self, op):
        spec = self.paths[op["name"]]
        inp = self._inputs(spec, op)
        e = self.e
        frag = self._step_refusal(spec)
        if frag is not None:         # refused before anything is launched: the handle is what it was
            self._refused(self._engine_call(spec, inp), frag)
            self._verify()
            return None
        ais = self.opt["apply_in_sweep"]
        if spec.get("apply_in_sweep", ais) != ais:       # a path that asks for its own setting: set for the call, then put back
            self.set_option("apply_in_sweep", spec["apply_in_sweep"])
        if spec["kind"] == "loop":
            evs = []
            for x in range(spec["n"]):
                ev = self._loop_event(inp["u_pick"], inp["u_def"], inp["u_np"], x)
                if ev is None:
                    break
                evs.append((ev.type, tuple(ev.pos), tuple(ev.target), ev.atom))
            self._verify()
            return dict(done=len(evs), status=int(len(evs) < spec["n"]), events=evs)
        staged = bool(op.get("staged") and self.staged)
        if spec["kind"] == "local":
            import local_ref
            ro = local_ref.run(self.o, self.lat, spec["step0"], spec["n"], DEFECT_FRACTION, COUNTER_SEED, spec["K"], spec["horizon"],
                               thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT)
            self._drop_marker()
            self.last = dict(max_per_box=ro["stats"]["max_per_box"])
            if e is not None:
                rg = e.run_supersteps_local(spec["step0"], spec["n"], DEFECT_FRACTION, COUNTER_SEED, spec["K"], spec["horizon"],
                                            thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT, want_events=True)
                self.check_local(e, self.lat, rg, ro, self.tag)
                self._verify_info()
            self.staged = None
            return ro
        if spec["kind"] == "run" and self._needs_stepper(op):
            ro, inp = self._stepper_run(op, spec, inp)
        else:
            ro = oracle_step(self.lat, spec, inp)
        if e is not None:
            if spec["kind"] == "run" and "resume" in op:        # the continuation of the batch that op["cut"] stopped
                x = op["resume"]
                kw = dict(rng_mode=spec["rng_mode"], seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT,
                          q_planes=inp["q"], incremental=spec["incremental"])
                rg = e.run_steps(spec["step0"] + x, spec["n"] - x, DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"], **kw)
                self.check_run(e, self.lat, rg, ro, self.tag)
            elif spec["kind"] == "run":
                kw = dict(rng_mode=spec["rng_mode"], seed=COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT,
                          q_planes=inp["q"], incremental=spec["incremental"])
                rg = e.run_steps(spec["step0"], spec["n"], DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"],
                                 staged=staged, **kw)
                if self._defers(spec):
                    self.deferred_expected += count_deferred([(spec["step0"], spec["n"])], spec["thermal_mode"])
                self.check_run(e, self.lat, rg, ro, self.tag)
            else:
                rg = e.run_supersteps(spec["step0"], spec["n"], spec["box"], DEFECT_FRACTION, COUNTER_SEED,
                                      thermal_mode=spec["thermal_mode"], thermal_dt=THERMAL_DT, q_planes=inp["q"], want_events=True,
                                      null_events=spec["null_events"])
                if spec["box"] == self.L and self._defers(dict(spec, incremental=False)):
                    self.deferred_expected += count_deferred([(spec["step0"], spec["n"])], spec["thermal_mode"])
                self.check_super(e, self.lat, rg, ro, self.tag)
            assert e.counters()["deferred_steps"] + self.deferred_reset == self.deferred_expected, \
                (self.tag, "deferred_steps", e.counters()["deferred_steps"], self.deferred_reset, self.deferred_expected)
            self._verify_info()
        self.staged = None
        if self.opt["apply_in_sweep"] != ais:
            self.set_option("apply_in_sweep", ais)
        return ro
