"""Sub-stepped temperature updates in the stepping loop (cetkmc_set_thermal_substeps + cetkmc_run_steps) against the comparator
tests/substep_ref.py after every call: stop state, stream positions, event log, totals (1e-11), counts, all five fields, the
row sums of the lattice the call left, q_used, and cetkmc_substep_info.  The inputs are tests/substep_cases.STEPPING (the
lattices and calls of tests/remelt_cases.py); tests/test_substep_ref_host.py asserts on the comparator alone what they
exercise."""
import numpy as np
import pytest

import remelt_cases as rc
import substep_cases as sc
from helpers import assert_call_matches_oracle
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1
MS_KEYS = ("ms_thermal", "ms_interface", "ms_sweep", "ms_dirty_rows", "ms_reduce", "ms_select_apply", "ms_comm")


def _engine(case, lat0, options=None, n_sub=None, n_slabs=1):
    import cetkmc
    e = cetkmc.Engine(case["L"], impurity_c=IMPURITY_C, n_slabs=n_slabs)
    for k, v in (sc.BLOCKED if options is None else options).items():      # small lattices: the blocked kernel by option
        e.set_option(k, v)
    e.upload(*lat0)
    if case.get("remelt"):
        e.set_remelt(True, case["threshold"])
    n_sub = case["n_sub"] if n_sub is None else n_sub
    if n_sub:
        e.set_thermal_substeps(n_sub)
    return e


def _run_call(e, case, call):
    s0, n, up, ud, unp, q = call
    return e.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"],
                       thermal_mode=case["thermal_mode"], q_planes=q, use_latent=case["use_latent"], incremental=case["incremental"])


def _blocked_per_update(n, S=sc.S_DEFAULT):
    return -(-(n - 1) // S)


def _check_case(oracle_mod, name, options=None, n_slabs=1):
    case = sc.STEPPING[name]
    run = sc.stepped(name)
    oracle_mod.set_threads(case["threads"])
    e = _engine(case, run["lat0"], options, n_slabs=n_slabs)
    try:
        updates = 0
        for c, call in enumerate(run["calls"]):
            rg = _run_call(e, case, call)
            lat = rc.LatView(run, c, IMPURITY_C)
            assert_call_matches_oracle(e, lat, rg, run["results"][c], RATE_RTOL, f"{name} {options or ''} call {c}")
            updates += updates_in(call[0], call[1])
            info = e.substep_info()
            assert (info["updates"], info["substeps"]) == (updates, updates * case["n_sub"]), (name, c, info)
        return e.counters(), info
    finally:
        e.close()
        oracle_mod.set_threads(1)


@pytest.mark.parametrize("name", [n for n in sc.STEPPING if not n.startswith(("L136", "L256"))])
def test_small_lattices_vs_comparator(oracle_mod, name):
    """L = 24 and 40 with the blocked kernel (option substep_block = 3, the default of larger lattices): rng_mode 0, 1, 2; full and incremental sweeps; thermal_mode 1 and 2 with and
    without latent heat; n = 3 and 17; remelting on in one L = 40 case (the melt follows the last sub-step)"""
    cnt, info = _check_case(oracle_mod, name)
    case = sc.STEPPING[name]
    assert (cnt["incremental_steps"] > 0) == case["incremental"]
    assert cnt["thermal_updates"] == info["updates"]                       # one update counts once
    per = _blocked_per_update(case["n_sub"])
    assert info["blocked_launches"] == info["updates"] * per and info["launches"] == info["updates"] * (1 + per)


@pytest.mark.parametrize("options", [dict(sc.BLOCKED, sweep_variant=0), dict(sc.BLOCKED, sweep_variant=1), dict(sc.BLOCKED, sweep_variant=3),
                                     dict(sc.BLOCKED, thermal_variant=0), dict(sc.BLOCKED, thermal_variant=2), {},
                                     {"substep_block": 1}, {"substep_block": 2, "substep_planes": 5}, {"substep_block": 4}],
                         ids=["sv0", "sv1", "sv3", "thermal_simple", "thermal_general", "default", "plain", "S2_planes5", "S4"])
def test_kernel_variants_vs_comparator(oracle_mod, options):
    """other sweep kernels behind the sub-stepped update, the one-thread-per-voxel temperature kernel (which takes the plain
    path), the handle's default (plain at this size), the plain path by option, two sub-steps per launch in plane groups of
    five and four per launch: same comparison"""
    cnt, info = _check_case(oracle_mod, "L24_laser_latent_rng0_full_n17", options)
    plain = options.get("thermal_variant") == 0 or options.get("substep_block", 1) == 1        # the default at L = 24 is plain
    assert (info["blocked_launches"] == 0) == plain
    assert info["launches"] == info["updates"] * (17 if plain else 1 + _blocked_per_update(17, options.get("substep_block", sc.S_DEFAULT)))


def test_three_slabs_vs_comparator(oracle_mod):
    """three in-process slabs at L = 24: n launches of the existing kernel, a halo exchange behind each"""
    cnt, info = _check_case(oracle_mod, "L24_laser_latent_rng0_full_n3", sc.BLOCKED, n_slabs=3)
    assert info["blocked_launches"] == 0 and info["launches"] == 3 * info["updates"]


def test_deferred_path_L136_vs_comparator(oracle_mod):
    cnt, info = _check_case(oracle_mod, "L136_laser_latent_deferred_n3", {})          # the handle's default: S = 3
    assert cnt["deferred_steps"] > 0 and info["blocked_launches"] == info["updates"] > 0


def test_fused_table_tiles_L256_vs_comparator(oracle_mod):
    """steps 19..41 at L = 256: sub-step 1 is the launch of the tiles that write the rate table; the table of the final field
    is written by k_rate_table before the sweep that follows"""
    cnt, info = _check_case(oracle_mod, "L256_fused_tiles_n3", {})
    assert cnt["thermal_updates"] == 2 == info["updates"] and info["blocked_launches"] == 2
    assert cnt["table_updates"] >= 2 + 2          # each update: the fused tiles, then k_rate_table for the last sub-step's field


def test_stream_shortage_on_an_update_step_applies_the_update_once(oracle_mod):
    """rng_mode 0: the batch runs out of its stream ON update step 20 (status 2) behind that step's n sub-steps; the
    continuation skips all of them"""
    from substep_ref import Stepper
    name = "L24_laser_latent_rng0_full_n17"
    case = sc.STEPPING[name]
    lat0 = rc.lattice_of(case)
    (s0, n, up, ud, unp, q), = rc.calls_of(dict(case, batches=(30,)))
    probe = Stepper(oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C), case["n_sub"])
    cut = probe.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=2, q_planes=q)["np_used"]
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = Stepper(lat, case["n_sub"])
    calls = [(0, 30, up, ud, unp[:cut], q), (20, 10, up[20:], ud[20:], unp, q[1:])]
    e = _engine(case, lat0)
    try:
        for c, call in enumerate(calls):
            ro = st.run_steps(call[0], call[1], 0.1, call[2], call[3], call[4], rng_mode=0, thermal_mode=2, q_planes=call[5])
            rg = _run_call(e, case, call)
            assert (ro["done"], ro["status"]) == ((20, 2), (10, 0))[c]
            assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"call {c}")
            info = e.substep_info()
            assert (info["updates"], info["substeps"]) == (2, 34) and st.stats["updates"] == 2       # updates 0 and 20, once each
    finally:
        e.close()


def test_termination_lets_the_queued_substeps_through(oracle_mod):
    """a lattice without events: status 1 at the first step; the updates queued behind it (blocked launches included) are
    pass-throughs that leave the field alone"""
    from substep_ref import Stepper
    L = 24
    case = dict(sc.STEPPING["L24_cet_rng1_incr_n3"], incremental=False, defect_fraction=0.0, n_sub=6)
    rs = np.random.RandomState(3)
    state = rs.randint(1, 5, (L, L, L)).astype(np.int64)
    ang = rs.random_sample((L, L, L))
    T = sc.noisy_gradient(L, seed=5)
    lat0 = (state, np.where(state < 4, ang, 0.0), np.where(state < 4, 2 * ang, 0.0), T, np.zeros_like(state))
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = Stepper(lat, 6)
    call = (0, 45, rs.random_sample(45), rs.random_sample(45), rs.random_sample(92), None)
    ro = st.run_steps(0, 45, 0.0, call[2], call[3], call[4], rng_mode=1, thermal_mode=1)
    assert (ro["done"], ro["status"]) == (0, 1) and st.stats["updates"] == 1
    e = _engine(case, lat0)
    try:
        rg = _run_call(e, case, call)
        assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, "terminated")
        assert e.substep_info()["updates"] == 3            # launches the host issued: the updates of steps 0, 20 and 40
    finally:
        e.close()


@pytest.mark.parametrize("name", ["L24_laser_latent_rng0_full_n3", "L136_laser_latent_deferred_n3"])
def test_one_substep_is_the_untouched_handle(name):
    """cetkmc_set_thermal_substeps(1): every bit, counter and launch count of the handle that never heard of it"""
    case = sc.STEPPING[name]
    lat0 = rc.lattice_of(case)
    calls = rc.calls_of(case)
    out = []
    for n_sub in (0, 1):                   # 0: the setter is not called (and no option is set)
        e = _engine(case, lat0, {}, n_sub=n_sub)
        try:
            res = [_run_call(e, case, call) for call in calls]
            cnt = e.counters()
            out.append((res, e.download(defects=True), {k: v for k, v in cnt.items() if k not in MS_KEYS}, e.substep_info(), e.rate_sweep(), e.row_sums()))
        finally:
            e.close()
    (r0, d0, c0, i0, s0, w0), (r1, d1, c1, i1, s1, w1) = out
    for a, b in zip(r0, r1):
        for f in ("done", "status", "np_used", "q_used", "nucleation_count", "full_sweeps", "sweep_launches", "min_margin"):
            assert a[f] == b[f], f
        for f in ("totals", "events", "n_events"):
            assert a[f].tobytes() == b[f].tobytes(), f
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert c0 == c1, {k: (c0[k], c1[k]) for k in c0 if c0[k] != c1[k]}
    assert s0 == s1 and w0[0].tobytes() == w1[0].tobytes() and w0[1].tobytes() == w1[1].tobytes()
    assert i0 == i1 == dict(updates=0, substeps=0, launches=0, blocked_launches=0)
