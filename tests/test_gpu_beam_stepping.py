"""A beam table in the stepping loop (cetkmc_set_beam + cetkmc_run_steps with thermal_mode 2 and no planes) against the comparator
tests/beam_ref.Stepper after every call: stop state, stream positions, event log, totals, counts, all five fields, the row sums,
q_used, cetkmc_get_beam_info and cetkmc_get_implicit_info.  The inputs are tests/beam_cases.STEPPING (implicit_cases' planted
lattices and calls under a serpentine scan whose second track begins inside the run); tests/test_beam_ref_host.py asserts on the
comparator alone what they exercise."""
import numpy as np
import pytest

import beam_cases as bm
import beam_ref
import implicit_cases as ic
import remelt_cases as rc
from helpers import assert_call_matches_oracle
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


def _engine(case, lat0, table=None):
    import cetkmc
    e = cetkmc.Engine(case["L"], impurity_c=IMPURITY_C)
    e.upload(*lat0)
    if case.get("remelt"):
        e.set_remelt(True, case["threshold"])
    if case["n_sub"] > 1:
        e.set_thermal_substeps(case["n_sub"])
    e.set_thermal_scheme("implicit")
    if case["bc"] is not None:
        e.set_thermal_boundary(case["bc"])
    e.set_beam(bm.table_of(case) if table is None else table)
    return e


def _run_call(e, case, call):
    s0, n, up, ud, unp, _ = call
    return e.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"],
                       thermal_mode=2, q_planes=None, use_latent=case["use_latent"], incremental=case["incremental"])


def _info(updates, n):
    return dict(updates=updates, steps=updates * n, launches=3 * updates * n, table_uploads=1)


def _check_case(oracle_mod, name):
    case = bm.STEPPING[name]
    run = bm.stepped(name)
    oracle_mod.set_threads(case["threads"])
    e = _engine(case, run["lat0"])
    try:
        updates = 0
        for c, call in enumerate(run["calls"]):
            rg = _run_call(e, case, call)
            lat = rc.LatView(run, c, IMPURITY_C)
            assert_call_matches_oracle(e, lat, rg, run["results"][c], RATE_RTOL, f"{name} call {c}")
            updates += updates_in(call[0], call[1])
            assert e.beam_info() == _info(updates, case["n_sub"]), (name, c)
            assert e.implicit_info()["updates"] == updates
            if case["bc"] is not None:
                assert e.boundary_info()["updates"] == updates
        if case.get("remelt"):
            assert e.remelt_info()["n_melted"] == run["stepper"].info["n_melted"] > 0
        return e.counters(), updates
    finally:
        e.close()
        oracle_mod.set_threads(1)


@pytest.mark.parametrize("name", [n for n in bm.STEPPING if not n.startswith("L136")])
def test_small_lattices_vs_comparator(oracle_mod, name):
    """L = 24 and 40: rng_mode 0, 1, 2; full and incremental sweeps; with and without latent heat; n = 1 and 3; depth 1, 2, 4;
    u0 = 2 from step0 = 40; remelting on at L = 40; the substrate sink in one case"""
    cnt, updates = _check_case(oracle_mod, name)
    case = bm.STEPPING[name]
    assert (cnt["incremental_steps"] > 0) == case["incremental"]
    assert cnt["thermal_updates"] == updates >= 2


def test_deferred_path_L136_vs_comparator(oracle_mod):
    cnt, updates = _check_case(oracle_mod, "L136_latent_deferred_n1_D2_sink")
    assert cnt["deferred_steps"] > 0 and updates > 0


def test_no_plane_crosses_to_the_device():
    """host-to-device bytes of a call: the uniforms alone (a plane call adds L * L * 8 per update)"""
    case = bm.STEPPING["L24_nolatent_rng1_incr_n1_D4"]
    e = _engine(case, ic.lattice_of(case))
    try:
        call = bm.calls_of(case)[0]
        b0 = e.counters()["bytes_h2d"]
        _run_call(e, case, call)
        n = call[1]
        assert e.counters()["bytes_h2d"] - b0 == 8 * n + 8 * n + 8 * call[4].size
    finally:
        e.close()


def test_stream_shortage_on_an_update_step_needs_nothing_supplied_again(oracle_mod):
    """rng_mode 0: the batch runs out of its stream ON update step 20 (status 2) behind that step's update; the continuation from
    step 20 supplies nothing but uniforms, skips that update, and the update of step 40 reads row 2"""
    case = bm.STEPPING["L24_latent_rng0_full_n3_D1_sink"]
    lat0 = ic.lattice_of(case)
    (s0, n, up, ud, unp, _), = bm.calls_of(dict(case, batches=(45,)))
    t = bm.table_of(dict(case, batches=(45,)))
    probe = beam_ref.Stepper(oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C), t, case["n_sub"], bc=case["bc"])
    # a step wants its candidates' draws and two orientation draws in the stream before it starts: two doubles past what steps
    # 0..19 consumed let step 19 run whatever its event drew, and leave step 20 (whose top plane holds candidates) short
    cut = probe.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=2)["np_used"] + 2
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = beam_ref.Stepper(lat, t, case["n_sub"], bc=case["bc"])
    calls = [(0, 45, up, ud, unp[:cut], None), (20, 25, up[20:], ud[20:], unp, None)]
    e = _engine(case, lat0, t)
    try:
        for c, call in enumerate(calls):
            ro = st.run_steps(call[0], call[1], 0.1, call[2], call[3], call[4], rng_mode=0, thermal_mode=2)
            rg = _run_call(e, case, call)
            assert (ro["done"], ro["status"]) == ((20, 2), (25, 0))[c]
            assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"call {c}")
        assert st.beam_updates == 3                                 # steps 0, 20 and 40, once each
        # the host's count is of what it issued: 0, 20 and (behind the stop, a pass-through) 40 in the first call, 40 in the second
        assert e.beam_info()["updates"] == 4
    finally:
        e.close()


def test_termination_lets_the_queued_updates_through(oracle_mod):
    """a lattice without events: status 1 at the first step; the beam updates queued behind it are pass-throughs"""
    L = 24
    case = dict(bm.STEPPING["L24_nolatent_rng1_incr_n1_D4"], incremental=False, defect_fraction=0.0, n_sub=2)
    rs = np.random.RandomState(3)
    state = rs.randint(1, 5, (L, L, L)).astype(np.int64)
    ang = rs.random_sample((L, L, L))
    T = rs.uniform(3000.0, 3600.0, (L, L, L))
    lat0 = (state, np.where(state < 4, ang, 0.0), np.where(state < 4, 2 * ang, 0.0), T, np.zeros_like(state))
    t = bm.scan_table(L, 0, 3, 4)
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = beam_ref.Stepper(lat, t, 2)
    call = (0, 45, rs.random_sample(45), rs.random_sample(45), rs.random_sample(92), None)
    ro = st.run_steps(0, 45, 0.0, call[2], call[3], call[4], rng_mode=1, thermal_mode=2, use_latent=False)
    assert (ro["done"], ro["status"]) == (0, 1) and st.beam_updates == 1
    e = _engine(case, lat0, t)
    try:
        rg = _run_call(e, case, call)
        assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, "terminated")
        assert e.beam_info()["updates"] == 3            # launches the host issued: the updates of steps 0, 20 and 40
    finally:
        e.close()


def test_one_call_equals_three_calls():
    """rng_mode 2 from step0 = 20: 46 steps in one call and cut at steps 27 and 40: every field, total and event equal"""
    case = dict(bm.STEPPING["L40_rng2_full_n1_remelt_D2"], step0=20)
    lat0 = ic.lattice_of(case)
    t = bm.table_of(dict(case, batches=(46,)))
    out = []
    for batches in ((46,), (7, 13, 26)):
        e = _engine(case, lat0, t)
        try:
            res = [_run_call(e, case, call) for call in bm.calls_of(dict(case, batches=batches))]
            out.append((np.concatenate([r["totals"] for r in res]), np.concatenate([r["events"] for r in res]), e.download(defects=True),
                        e.beam_info()))
        finally:
            e.close()
    (t0, e0, d0, i0), (t1, e1, d1, i1) = out
    assert t0.tobytes() == t1.tobytes() and e0.tobytes() == e1.tobytes()
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert i0 == i1 and i0["updates"] == 3
