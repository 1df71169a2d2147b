"""A thermal boundary in the stepping loop (cetkmc_set_thermal_boundary + cetkmc_run_steps) against the comparator
tests/boundary_ref.Stepper after every call: stop state, stream positions, event log, totals, counts, all five fields, the row
sums, q_used, cetkmc_get_thermal_boundary's totals and cetkmc_get_implicit_info.  The inputs are tests/boundary_cases.STEPPING
(implicit_cases' planted lattices and calls with the gradient boundary in thermal_mode 1 and the substrate sink in thermal_mode
2); tests/test_boundary_ref_host.py asserts on the comparator alone what they exercise."""
import numpy as np
import pytest

import boundary_cases as bc
import boundary_ref as br
import implicit_cases as ic
import remelt_cases as rc
from helpers import assert_call_matches_oracle
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


def _engine(case, lat0, boundary="case"):
    import cetkmc
    e = cetkmc.Engine(case["L"], impurity_c=IMPURITY_C)
    e.upload(*lat0)
    if case.get("remelt"):
        e.set_remelt(True, case["threshold"])
    if case["n_sub"] > 1:
        e.set_thermal_substeps(case["n_sub"])
    e.set_thermal_scheme("implicit")
    e.set_thermal_boundary(bc._bc_of(case) if boundary == "case" else boundary)
    return e


def _run_call(e, case, call):
    s0, n, up, ud, unp, q = call
    return e.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"],
                       thermal_mode=case["thermal_mode"], q_planes=q, use_latent=case["use_latent"], incremental=case["incremental"])


def _infos(updates, n):
    return (dict(updates=updates, steps=updates * n, launches=3 * updates * n, coeff_uploads=min(updates, 1)),
            dict(updates=updates, steps=updates * n, launches=3 * updates * n, coeff_uploads=0))


def _check_case(oracle_mod, name):
    case = bc.STEPPING[name]
    run = bc.stepped(name)
    oracle_mod.set_threads(case["threads"])
    e = _engine(case, run["lat0"])
    try:
        updates = 0
        for c, call in enumerate(run["calls"]):
            rg = _run_call(e, case, call)
            lat = rc.LatView(run, c, IMPURITY_C)
            assert_call_matches_oracle(e, lat, rg, run["results"][c], RATE_RTOL, f"{name} call {c}")
            updates += updates_in(call[0], call[1])
            assert (e.boundary_info(), e.implicit_info()) == _infos(updates, case["n_sub"]), (name, c)
        return e.counters(), updates
    finally:
        e.close()
        oracle_mod.set_threads(1)


@pytest.mark.parametrize("name", [n for n in bc.STEPPING if not n.startswith("L136")])
def test_small_lattices_vs_comparator(oracle_mod, name):
    """L = 24 and 40: rng_mode 0, 1, 2; full and incremental sweeps; thermal_mode 1 with the gradient boundary, thermal_mode 2
    with the sink under a moving source, with and without latent heat; n = 1 and 3; remelting on in one L = 40 case; a ramp of
    -200 K per update from step0 = 40 with calls that end at steps 47, 60, 61, 81"""
    cnt, updates = _check_case(oracle_mod, name)
    case = bc.STEPPING[name]
    assert (cnt["incremental_steps"] > 0) == case["incremental"]
    assert cnt["thermal_updates"] == updates >= 2


def test_deferred_path_L136_vs_comparator(oracle_mod):
    cnt, updates = _check_case(oracle_mod, "L136_laser_latent_deferred_n1_sink")
    assert cnt["deferred_steps"] > 0 and updates > 0


def test_one_call_equals_three_calls_with_a_ramp():
    """rng_mode 2 from step0 = 20: 46 steps in one call and cut at steps 27 and 40 (27 is no multiple of 20; the call that begins at
    40 begins on an update): every field, total and event equal, bit for bit"""
    case = dict(bc.STEPPING["L40_cet_rng2_full_n3_ramp"], step0=20)
    lat0 = ic.lattice_of(case)
    out = []
    for batches in ((46,), (7, 13, 26)):
        e = _engine(case, lat0)
        try:
            res = [_run_call(e, case, call) for call in rc.calls_of(dict(case, batches=batches))]
            out.append((np.concatenate([r["totals"] for r in res]), np.concatenate([r["events"] for r in res]), e.download(defects=True),
                        e.boundary_info()))
        finally:
            e.close()
    (t0, e0, d0, i0), (t1, e1, d1, i1) = out
    assert t0.tobytes() == t1.tobytes() and e0.tobytes() == e1.tobytes()
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert i0 == i1 and i0["updates"] == 3


def test_stream_shortage_on_an_update_step_applies_the_update_once(oracle_mod):
    """rng_mode 0, the sink with a ramp: the batch runs out of its stream ON update step 20 (status 2) behind that step's update;
    the continuation skips it, and the update of step 40 uses u = 2"""
    case = dict(bc.STEPPING["L24_laser_latent_rng0_full_n3_sink"], bc=bc.sink(bc.COOLING))
    lat0 = ic.lattice_of(case)
    (s0, n, up, ud, unp, q), = rc.calls_of(dict(case, batches=(45,)))
    probe = br.Stepper(oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C), case["n_sub"], bc=case["bc"])
    cut = probe.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=2, q_planes=q)["np_used"]
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = br.Stepper(lat, case["n_sub"], bc=case["bc"])
    calls = [(0, 45, up, ud, unp[:cut], q), (20, 25, up[20:], ud[20:], unp, q[1:])]
    e = _engine(case, lat0)
    try:
        for c, call in enumerate(calls):
            ro = st.run_steps(call[0], call[1], 0.1, call[2], call[3], call[4], rng_mode=0, thermal_mode=2, q_planes=call[5])
            rg = _run_call(e, case, call)
            assert (ro["done"], ro["status"]) == ((20, 2), (25, 0))[c]
            assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"call {c}")
        assert st.bc_updates == 3                                  # steps 0, 20 and 40, once each
        # the host's count is of what it issued: 0, 20 and (behind the stop, a pass-through) 40 in the first call, 40 in the second
        assert e.boundary_info()["updates"] == 4
    finally:
        e.close()


def test_termination_lets_the_queued_updates_through(oracle_mod):
    """a lattice without events: status 1 at the first step; the boundary updates queued behind it are pass-throughs"""
    L = 24
    case = dict(bc.STEPPING["L24_cet_rng1_incr_n3_gradient"], incremental=False, defect_fraction=0.0, n_sub=2)
    rs = np.random.RandomState(3)
    state = rs.randint(1, 5, (L, L, L)).astype(np.int64)
    ang = rs.random_sample((L, L, L))
    T = rs.uniform(3000.0, 3600.0, (L, L, L))
    lat0 = (state, np.where(state < 4, ang, 0.0), np.where(state < 4, 2 * ang, 0.0), T, np.zeros_like(state))
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = br.Stepper(lat, 2, bc=bc.gradient(L))
    call = (0, 45, rs.random_sample(45), rs.random_sample(45), rs.random_sample(92), None)
    ro = st.run_steps(0, 45, 0.0, call[2], call[3], call[4], rng_mode=1, thermal_mode=1)
    assert (ro["done"], ro["status"]) == (0, 1) and st.stats["updates"] == 1
    e = _engine(case, lat0)
    try:
        rg = _run_call(e, case, call)
        assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, "terminated")
        assert e.boundary_info()["updates"] == 3            # launches the host issued: the updates of steps 0, 20 and 40
    finally:
        e.close()
