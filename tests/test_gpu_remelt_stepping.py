"""Remelting in the stepping loop (cetkmc_set_remelt + cetkmc_run_steps) against the comparator tests/remelt_ref.py after every
call: stop state, stream positions, event log, totals (1e-11), counts, all five fields, the row sums of the lattice the call
left, q_used and cetkmc_remelt_info.  The inputs are tests/remelt_cases.STEPPING; tests/test_remelt_ref_host.py asserts on the
comparator alone that each of them melts at two or more updates, refills a melted voxel and melts listed, interior and state-4
voxels."""
import numpy as np
import pytest

import remelt_cases as rc
from helpers import assert_call_matches_oracle
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1
MS_KEYS = ("ms_thermal", "ms_interface", "ms_sweep", "ms_dirty_rows", "ms_reduce", "ms_select_apply", "ms_comm")


def _engine(case, lat0, options=None, remelt=True):
    import cetkmc
    e = cetkmc.Engine(case["L"], impurity_c=IMPURITY_C)
    for k, v in (options or {}).items():
        e.set_option(k, v)
    e.upload(*lat0)
    if remelt:
        e.set_remelt(True, case["threshold"])
    return e


def _run_call(e, case, call):
    s0, n, up, ud, unp, q = call
    return e.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"],
                       thermal_mode=case["thermal_mode"], q_planes=q, use_latent=case["use_latent"], incremental=case["incremental"])


def _check_case(oracle_mod, name, options=None):
    case = rc.STEPPING[name]
    run = rc.stepped(name)
    oracle_mod.set_threads(case["threads"])
    e = _engine(case, run["lat0"], options)
    try:
        for c, call in enumerate(run["calls"]):
            rg = _run_call(e, case, call)
            lat = rc.LatView(run, c, IMPURITY_C)
            ro = run["results"][c]
            assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"{name} {options or ''} call {c}")
            info = e.remelt_info()
            assert {k: info[k] for k in ("passes", "n_melted", "n_melted_last")} == run["infos"][c], (name, c, info, run["infos"][c])
            assert 0 <= info["n_appended"] <= case["L"] ** 3
        return e.counters()
    finally:
        e.close()
        oracle_mod.set_threads(1)


@pytest.mark.parametrize("name", [n for n in rc.STEPPING if not n.startswith(("L136", "L256"))])
def test_small_lattices_vs_comparator(oracle_mod, name):
    """L = 24, 40, 64 with the handle's defaults (the library has no getter for the sweep kernel it picks at L <= 128;
    test_sweep_variants_vs_comparator pins variants 0, 1, 3 and 4 by option); rng_mode 0, 1, 2; full and incremental; thermal_mode 1 with a lowered
    threshold, 2 with and without latent heat under a moving source; defect_fraction up to 0.1"""
    cnt = _check_case(oracle_mod, name)
    case = rc.STEPPING[name]
    assert (cnt["incremental_steps"] > 0) == case["incremental"]
    assert cnt["deferred_steps"] == 0


@pytest.mark.parametrize("options", [{"sweep_variant": 0}, {"sweep_variant": 1}, {"sweep_variant": 3}, {"sweep_variant": 4},
                                     {"interface_every_step": 1}, {"thermal_variant": 0}],
                         ids=["sv0", "sv1", "sv3", "sv4", "ifc_every_step", "thermal_simple"])
def test_sweep_variants_vs_comparator(oracle_mod, options):
    """the straightforward sweep (no rate table, no interface sums) against the streaming ones, the interface kernel before
    every sweep, and the one-thread-per-voxel temperature kernel: same comparison"""
    _check_case(oracle_mod, "L24_laser_latent_rng0_full", options)


def test_deferred_path_L136_vs_comparator(oracle_mod):
    cnt = _check_case(oracle_mod, "L136_laser_latent_deferred")
    assert cnt["deferred_steps"] > 0


def test_fused_table_tiles_L256_vs_comparator(oracle_mod):
    """steps 19..41 at L = 256: the temperature tiles that write the rate table, then the melt, then the interface kernel"""
    cnt = _check_case(oracle_mod, "L256_fused_tiles")
    assert cnt["table_updates"] == 2 + 1 and cnt["thermal_updates"] == 2      # the call's first sweep and the two fused updates


def test_stream_shortage_on_an_update_step_counts_the_pass_once(oracle_mod):
    """rng_mode 0: the batch runs out of its stream ON update step 20 (status 2) behind that step's update and melt; the
    continuation skips both"""
    from remelt_ref import Stepper
    name = "L24_laser_latent_rng0_full"
    case = rc.STEPPING[name]
    lat0 = rc.lattice_of(case)
    (s0, n, up, ud, unp, q), = rc.calls_of(dict(case, batches=(30,)))
    probe = Stepper(oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C), case["threshold"])
    cut = probe.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=2, q_planes=q)["np_used"]
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = Stepper(lat, case["threshold"])
    calls = [(0, 30, up, ud, unp[:cut], q), (20, 10, up[20:], ud[20:], unp, q[1:])]
    e = _engine(case, lat0)
    try:
        for c, call in enumerate(calls):
            ro = st.run_steps(call[0], call[1], 0.1, call[2], call[3], call[4], rng_mode=0, thermal_mode=2, q_planes=call[5])
            rg = _run_call(e, case, call)
            assert (ro["done"], ro["status"]) == ((20, 2), (10, 0))[c]
            assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"call {c}")
            info = e.remelt_info()
            assert {k: info[k] for k in st.info} == st.info, (c, info, st.info)
            assert info["passes"] == 2 and st.info["n_melted_last"] > 0          # updates 0 and 20, once each
    finally:
        e.close()


def test_termination_lets_the_queued_passes_through(oracle_mod):
    """a lattice without events (every voxel occupied, nothing at or above the threshold): status 1 at the first step; the
    updates and melts queued behind it are pass-throughs, so one pass is counted"""
    from remelt_ref import Stepper
    L = 24
    case = dict(rc.STEPPING["L24_laser_nolatent_rng1_incr"], thermal_mode=1, incremental=False, defect_fraction=0.0)
    rs = np.random.RandomState(3)
    state = rs.randint(1, 5, (L, L, L)).astype(np.int64)
    ang = rs.random_sample((L, L, L))
    lat0 = (state, np.where(state < 4, ang, 0.0), np.where(state < 4, 2 * ang, 0.0), np.full((L, L, L), 3690.0), np.zeros_like(state))
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = Stepper(lat, case["threshold"])
    call = (0, 45, rs.random_sample(45), rs.random_sample(45), rs.random_sample(92), None)
    ro = st.run_steps(0, 45, 0.0, call[2], call[3], call[4], rng_mode=1, thermal_mode=1)
    assert (ro["done"], ro["status"]) == (0, 1) and st.info == dict(passes=1, n_melted=0, n_melted_last=0)
    e = _engine(case, lat0)
    try:
        rg = _run_call(e, case, call)
        assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, "terminated")
        assert e.remelt_info() == dict(passes=1, n_melted=0, n_melted_last=0, n_appended=0)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["L24_laser_latent_rng0_full", "L64_laser_latent_rng1_incr", "L136_laser_latent_deferred"])
def test_threshold_inf_is_the_run_without_remelting(oracle_mod, name):
    """a threshold of +inf: every bit, counter and launch count of the run with remelting off, except passes"""
    case = rc.STEPPING[name]
    lat0 = rc.lattice_of(case)
    calls = rc.calls_of(case)
    out = []
    for on in (False, True):
        e = _engine(dict(case, threshold=np.inf), lat0, remelt=on)
        try:
            res = [_run_call(e, case, call) for call in calls]
            cnt = e.counters()
            out.append((res, e.download(defects=True), {k: v for k, v in cnt.items() if k not in MS_KEYS}, e.remelt_info(), e.rate_sweep(), e.row_sums()))
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
    n_updates = sum(1 for (s, n, *_) in calls for g in range(s, s + n) if g % 20 == 0)
    assert i0 == dict(passes=0, n_melted=0, n_melted_last=0, n_appended=0)
    assert i1 == dict(passes=n_updates, n_melted=0, n_melted_last=0, n_appended=0)
