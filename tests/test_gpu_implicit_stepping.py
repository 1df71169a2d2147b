"""The implicit scheme in the stepping loop (cetkmc_set_thermal_scheme + cetkmc_run_steps) against the comparator
tests/implicit_ref.Stepper after every call: stop state, stream positions, event log, totals (1e-11), counts, all five fields,
the row sums of the lattice the call left, q_used, and cetkmc_get_implicit_info.  The inputs are
tests/implicit_cases.STEPPING (the lattices and calls of tests/remelt_cases.py, every case beginning on an update step, with a
NaN, a +inf, a block below T_clip_lo and a block above T_clip_hi in the field); tests/test_implicit_ref_host.py asserts on the comparator alone what they exercise."""
import numpy as np
import pytest

import implicit_cases as ic
import remelt_cases as rc
from helpers import assert_call_matches_oracle
from implicit_ref import Stepper
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1
MS_KEYS = ("ms_thermal", "ms_interface", "ms_sweep", "ms_dirty_rows", "ms_reduce", "ms_select_apply", "ms_comm")


def _engine(case, lat0, scheme="implicit", n_sub=None):
    import cetkmc
    e = cetkmc.Engine(case["L"], impurity_c=IMPURITY_C)
    e.upload(*lat0)
    if case.get("remelt"):
        e.set_remelt(True, case["threshold"])
    n_sub = case["n_sub"] if n_sub is None else n_sub
    if n_sub > 1:
        e.set_thermal_substeps(n_sub)
    if scheme is not None:
        e.set_thermal_scheme(scheme)
    return e


def _run_call(e, case, call):
    s0, n, up, ud, unp, q = call
    return e.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"],
                       thermal_mode=case["thermal_mode"], q_planes=q, use_latent=case["use_latent"], incremental=case["incremental"])


def _check_case(oracle_mod, name):
    case = ic.STEPPING[name]
    run = ic.stepped(name)
    oracle_mod.set_threads(case["threads"])
    e = _engine(case, run["lat0"])
    try:
        updates = 0
        for c, call in enumerate(run["calls"]):
            rg = _run_call(e, case, call)
            lat = rc.LatView(run, c, IMPURITY_C)
            assert_call_matches_oracle(e, lat, rg, run["results"][c], RATE_RTOL, f"{name} call {c}")
            updates += updates_in(call[0], call[1])
            info = e.implicit_info()
            assert info == dict(updates=updates, steps=updates * case["n_sub"], launches=3 * updates * case["n_sub"],
                                coeff_uploads=min(updates, 1)), (name, c, info)
        return e.counters(), info
    finally:
        e.close()
        oracle_mod.set_threads(1)


@pytest.mark.parametrize("name", [n for n in ic.STEPPING if not n.startswith(("L136", "L256"))])
def test_small_lattices_vs_comparator(oracle_mod, name):
    """L = 24 and 40: rng_mode 0, 1, 2; full and incremental sweeps; thermal_mode 1 and 2 with and without latent heat under a
    moving source; n = 1 and 3; remelting on in one L = 40 case (the melt follows the update)"""
    cnt, info = _check_case(oracle_mod, name)
    case = ic.STEPPING[name]
    assert (cnt["incremental_steps"] > 0) == case["incremental"]
    assert cnt["thermal_updates"] == info["updates"]                       # one update counts once


def test_deferred_path_L136_vs_comparator(oracle_mod):
    cnt, info = _check_case(oracle_mod, "L136_laser_latent_deferred_n1")
    assert cnt["deferred_steps"] > 0 and info["updates"] > 0


def test_L256_vs_comparator(oracle_mod):
    """steps 20..42 at L = 256: the implicit launches replace the tiles that write the rate table; k_rate_table writes the table
    of the final field before the sweep that follows"""
    cnt, info = _check_case(oracle_mod, "L256_fused_tiles_n1")
    assert cnt["thermal_updates"] == 2 == info["updates"]
    assert cnt["table_updates"] >= 2


def test_stream_shortage_on_an_update_step_applies_the_update_once(oracle_mod):
    """rng_mode 0: the batch runs out of its stream ON update step 20 (status 2) behind that step's implicit steps; the
    continuation skips all of them"""
    name = "L24_laser_latent_rng0_full_n3"
    case = ic.STEPPING[name]
    lat0 = ic.lattice_of(case)
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
            info = e.implicit_info()
            assert (info["updates"], info["steps"]) == (2, 6) and st.stats["updates"] == 2       # updates 0 and 20, once each
    finally:
        e.close()


def test_termination_lets_the_queued_updates_through(oracle_mod):
    """a lattice without events: status 1 at the first step; the updates queued behind it are pass-throughs (k_imp_rows copies,
    k_imp_lines returns) that leave the field alone"""
    L = 24
    case = dict(ic.STEPPING["L24_cet_rng1_incr_n3"], incremental=False, defect_fraction=0.0, n_sub=2)
    rs = np.random.RandomState(3)
    state = rs.randint(1, 5, (L, L, L)).astype(np.int64)
    ang = rs.random_sample((L, L, L))
    T = rs.uniform(3000.0, 3600.0, (L, L, L))
    lat0 = (state, np.where(state < 4, ang, 0.0), np.where(state < 4, 2 * ang, 0.0), T, np.zeros_like(state))
    lat = oracle_mod.Lattice(*lat0, impurity_c=IMPURITY_C)
    st = Stepper(lat, 2)
    call = (0, 45, rs.random_sample(45), rs.random_sample(45), rs.random_sample(92), None)
    ro = st.run_steps(0, 45, 0.0, call[2], call[3], call[4], rng_mode=1, thermal_mode=1)
    assert (ro["done"], ro["status"]) == (0, 1) and st.stats["updates"] == 1
    e = _engine(case, lat0)
    try:
        rg = _run_call(e, case, call)
        assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, "terminated")
        assert e.implicit_info()["updates"] == 3           # launches the host issued: the updates of steps 0, 20 and 40
    finally:
        e.close()


@pytest.mark.parametrize("name", ["L24_laser_latent_rng0_full_n3", "L136_laser_latent_deferred_n1"])
def test_scheme_set_to_explicit_is_the_untouched_handle(name):
    """cetkmc_set_thermal_scheme(explicit): every bit, counter and launch count of the handle that never heard of it"""
    case = ic.STEPPING[name]
    lat0 = rc.lattice_of(case)
    calls = rc.calls_of(case)
    out = []
    for scheme in (None, "explicit"):
        e = _engine(case, lat0, scheme=scheme)
        try:
            res = [_run_call(e, case, call) for call in calls]
            cnt = e.counters()
            out.append((res, e.download(defects=True), {k: v for k, v in cnt.items() if k not in MS_KEYS}, e.substep_info(), e.implicit_info(),
                        e.rate_sweep(), e.row_sums()))
        finally:
            e.close()
    (r0, d0, c0, b0, i0, s0, w0), (r1, d1, c1, b1, i1, s1, w1) = out
    for a, b in zip(r0, r1):
        for f in ("done", "status", "np_used", "q_used", "nucleation_count", "full_sweeps", "sweep_launches", "min_margin"):
            assert a[f] == b[f], f
        for f in ("totals", "events", "n_events"):
            assert a[f].tobytes() == b[f].tobytes(), f
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert c0 == c1, {k: (c0[k], c1[k]) for k in c0 if c0[k] != c1[k]}
    assert s0 == s1 and w0[0].tobytes() == w1[0].tobytes() and w0[1].tobytes() == w1[1].tobytes()
    assert b0 == b1 and i0 == i1 == dict(updates=0, steps=0, launches=0, coeff_uploads=0)


def test_back_to_explicit_in_the_loop_is_the_untouched_handle():
    """one handle makes its first call under the implicit scheme, the other under the explicit one; both are then given the same
    fields again and step 25 Mode A steps with an update in them: equal in every bit and in every counter of that call"""
    case = ic.STEPPING["L24_laser_latent_rng0_full_n1"]
    lat0 = rc.lattice_of(case)
    (c_a, c_b) = rc.calls_of(dict(case, batches=(10, 25)))
    out = []
    for scheme in ("implicit", None):
        e = _engine(case, lat0, scheme=scheme)
        try:
            _run_call(e, case, c_a)
            if scheme:
                e.set_thermal_scheme("explicit")
            e.upload(*lat0)
            c0 = e.counters()
            r = _run_call(e, case, c_b)
            c1 = e.counters()
            out.append((r, e.download(defects=True), {k: c1[k] - c0[k] for k in c1 if k not in MS_KEYS}, e.rate_sweep()))
        finally:
            e.close()
    (r0, d0, c0, s0), (r1, d1, c1, s1) = out
    # (nucleation_count runs over the handle's life: the first calls, under different schemes, may have nucleated differently)
    for f in ("done", "status", "np_used", "q_used", "full_sweeps", "sweep_launches", "min_margin"):
        assert r0[f] == r1[f], f
    for f in ("totals", "events", "n_events"):
        assert r0[f].tobytes() == r1[f].tobytes(), f
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert c0 == c1, {k: (c0[k], c1[k]) for k in c0 if c0[k] != c1[k]}
    assert s0 == s1
