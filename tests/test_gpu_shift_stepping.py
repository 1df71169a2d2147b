"""cetkmc_shift between stepping calls, against the oracle after every call (helpers.assert_call_matches_oracle): the oracle --
or the comparator stepper that drives it where the oracle has no such temperature update -- receives the fields of the
comparator tests/shift_ref.py, with prev_state := state as behind an upload.

  L = 16        all three rng_modes x incremental and full sweeps x thermal modes 0, 1, 2; two shifts between three calls
  L = 136       the deferred path (cetkmc_counters.deferred_steps > 0), laser planes
  L = 24        implicit scheme + a heat-sink boundary + a beam table, three sub-steps (beam_ref.Stepper); in the same run a call
                that stops with status 2 ON update step 20, a shift behind it, and the continuation from step 20, which applies
                that step's update again as it does behind an upload
  L = 40        remelting on, counter uniforms
  L = 16        a shift behind a termination; a staged batch consumed behind a shift

A twin handle goes through download, comparator and upload in place of every shift: over the 40 steps that follow it agrees with
the first handle bit for bit -- totals, events, all five fields.

Asserted on the oracle's log alone: the call behind every shift executes at least one event in an exposed voxel or within two
voxels of the seam between exposed and kept voxels."""
import numpy as np
import pytest

import beam_cases as bm
import beam_ref
import implicit_cases as ic
import shift_ref as SR
from shift_cases import events_in_zone
from helpers import (FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, face_lattice, oracle_lattice, random_lattice)
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
SHIFT_A = dict(d=(-4, 0, 0), fill_state=0, fill_T=3000.0, T_mode="value", fill_theta=0.0, fill_phi=0.0)      # a recoated layer
SHIFT_B = dict(d=(0, 3, -2), fill_state=1, fill_T=0.0, T_mode="edge", fill_theta=0.3, fill_phi=1.1)          # a frame that moves


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def shift_oracle(lat, d, **kw):
    """the comparator's fields into the oracle lattice, as an upload of all five would leave them"""
    out, info = SR.shift_fields(dict(state=lat.state, defects=lat.defects, theta=lat.theta, phi=lat.phi, T=lat.T), d, **kw)
    lat.state = np.ascontiguousarray(out["state"], dtype=np.int8)
    lat.defects = np.ascontiguousarray(out["defects"], dtype=np.int8)
    lat.theta, lat.phi, lat.T = (np.ascontiguousarray(out[k], dtype=np.float64) for k in ("theta", "phi", "T"))
    lat.prev_state = lat.state.copy()
    return info


def shift_by_host(e, d, **kw):
    """what the parent offers: download, comparator, upload"""
    out, _ = SR.shift_fields(e.download(defects=True), d, **kw)
    e.upload(out["state"], out["theta"], out["phi"], out["T"], out["defects"])


def assert_twins_agree(rg, rg2, e, e2, tag):
    assert (rg["done"], rg["status"], rg["np_used"], rg["nucleation_count"]) == (rg2["done"], rg2["status"], rg2["np_used"], rg2["nucleation_count"]), tag
    assert np.array_equal(_bits(rg["totals"]), _bits(rg2["totals"])), tag
    assert rg["events"].tobytes() == rg2["events"].tobytes(), tag
    a, b = e.download(defects=True), e2.download(defects=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (tag, k)


def _engines(L, lat, tweak=None, planes=False):
    import cetkmc
    out = []
    for _ in range(2):
        params = cetkmc.default_params(IMPURITY_C)
        for k, v in (tweak or {}).items():
            setattr(params, k, v)
        e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
        if planes:
            e.upload_planes(0, L, *lat)
            e.set_prev_state(None)
        else:
            e.upload(*lat)
        out.append(e)
    return out


@pytest.mark.parametrize("thermal_mode", [0, 1, 2])
@pytest.mark.parametrize("incremental", [False, True])
@pytest.mark.parametrize("rng_mode", [0, 1, 2])
def test_shifts_between_calls_vs_oracle(oracle_mod, rng_mode, incremental, thermal_mode):
    from cetkmc import synthetic
    L = 16
    lat = random_lattice(L, 31)
    e, e2 = _engines(L, lat, FOUR_KIND_PARAMS)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    try:
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(batch_calls((25, 40, 40))):
            tag = f"rng_mode {rng_mode} incremental {incremental} thermal_mode {thermal_mode} call {c}"
            sh = (None, SHIFT_A, SHIFT_B)[c]
            if sh is not None:
                info = e.shift(**sh)
                assert info == dict(shift_oracle(o, **sh), calls=c), tag
                shift_by_host(e2, **sh)
            if rng_mode == 0:
                u_np = np.random.RandomState(c).random_sample(n * (L * L + 2))
            q = synthetic.laser_planes(L, step0, n) if thermal_mode == 2 else None
            kw = dict(rng_mode=rng_mode, seed=5, thermal_mode=thermal_mode, q_planes=q)
            rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, incremental=incremental, **kw)
            rg2 = e2.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, incremental=incremental, **kw)
            if rng_mode == 2:      # all-counter uniforms: the oracle's single-domain super-steps are these steps
                ro = o.run_supersteps(step0, n, L, DEFECT_FRACTION, 5, thermal_mode=thermal_mode, q_planes=q)
                ro = dict(ro, events=ro["events"][:, 0])
            else:
                ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            assert (ro["done"], ro["status"]) == (n, 0), tag
            assert sh is None or events_in_zone(L, sh["d"], ro["events"]) >= 1, tag
            assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag)
            assert_twins_agree(rg, rg2, e, e2, tag)
        assert (e.counters()["incremental_steps"] > 0) == incremental
    finally:
        e.close()
        e2.close()


def test_deferred_path_L136_vs_oracle(oracle_mod):
    from cetkmc import synthetic
    L = 136
    lat = face_lattice(L, 17 + L, 6000)
    e, e2 = _engines(L, lat, FOUR_KIND_PARAMS, planes=True)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    oracle_mod.set_threads(16)
    sh = dict(d=(-8, 0, 0), fill_state=0, fill_T=3200.0, T_mode="value", fill_theta=0.0, fill_phi=0.0)
    try:
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(batch_calls((25, 40))):
            if c == 1:
                assert e.shift(**sh) == dict(shift_oracle(o, **sh), calls=1)
                shift_by_host(e2, **sh)
            q = synthetic.laser_planes(L, step0, n)
            kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=q)
            rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            assert (ro["done"], ro["status"]) == (n, 0)
            assert c == 0 or events_in_zone(L, sh["d"], ro["events"]) >= 1
            assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, f"L=136 call {c}")
            if c == 1:
                assert_twins_agree(rg, e2.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw), e, e2, "L=136")
            else:
                e2.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
        d0 = e.counters()["deferred_steps"]
        assert d0 > 30
    finally:
        oracle_mod.set_threads(1)
        e.close()
        e2.close()


def _beam_engine(case, lat0, table):
    import cetkmc
    e = cetkmc.Engine(case["L"], impurity_c=0.1)
    e.upload(*lat0)
    if case.get("remelt"):
        e.set_remelt(True, case["threshold"])
    if case["n_sub"] > 1:
        e.set_thermal_substeps(case["n_sub"])
    e.set_thermal_scheme("implicit")
    if case["bc"] is not None:
        e.set_thermal_boundary(case["bc"])
    e.set_beam(table)
    return e


def _beam_call(e, case, call):
    s0, n, up, ud, unp, _ = call
    return e.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"], thermal_mode=2,
                       q_planes=None, use_latent=case["use_latent"], incremental=case["incremental"])


def test_implicit_boundary_beam_and_a_stop_on_an_update_step(oracle_mod):
    """L = 24, rng_mode 0, n = 3, the substrate sink, a beam of depth 1.  Call 0 runs out of its stream ON step 20, behind that
    step's update (status 2); both are shifted; the continuation from step 20 applies the update of step 20 once more -- the
    handle forgot it, as behind an upload -- and the comparator, told the same, agrees."""
    case = bm.STEPPING["L24_latent_rng0_full_n3_D1_sink"]
    L = case["L"]
    lat0 = ic.lattice_of(case)
    (s0, n, up, ud, unp, _), = bm.calls_of(dict(case, batches=(65,)))
    t = bm.table_of(dict(case, batches=(65,)))
    probe = beam_ref.Stepper(oracle_mod.Lattice(*lat0, impurity_c=0.1), t, case["n_sub"], bc=case["bc"])
    cut = probe.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=2)["np_used"] + 2
    lat = oracle_mod.Lattice(*lat0, impurity_c=0.1)
    st = beam_ref.Stepper(lat, t, case["n_sub"], bc=case["bc"])
    calls = [(0, 45, up, ud, unp[:cut], None), (20, 45, up[20:], ud[20:], unp, None)]
    e, e2 = _beam_engine(case, lat0, t), _beam_engine(case, lat0, t)
    sh = dict(SHIFT_A, fill_T=3100.0)
    try:
        for c, call in enumerate(calls):
            if c == 1:
                assert e.shift(**sh) == dict(shift_oracle(lat, **sh), calls=1)
                st.applied_g = -1                       # a new field: the applied update is no longer remembered
                shift_by_host(e2, **sh)
            ro = st.run_steps(call[0], call[1], 0.1, call[2], call[3], call[4], rng_mode=0, thermal_mode=2)
            rg, rg2 = _beam_call(e, case, call), _beam_call(e2, case, call)
            assert (ro["done"], ro["status"]) == ((20, 2), (45, 0))[c]
            assert c == 0 or events_in_zone(L, sh["d"], ro["events"]) >= 1
            assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"call {c}")
            assert_twins_agree(rg, rg2, e, e2, f"call {c}")
        assert st.beam_updates == 5                     # steps 0 and 20, then 20 again, 40 and 60
        assert e.thermal_boundary() == e2.thermal_boundary() and e.implicit_info() == e2.implicit_info() and e.beam_info() == e2.beam_info()
    finally:
        e.close()
        e2.close()


def test_remelting_on(oracle_mod):
    case = bm.STEPPING["L40_rng2_full_n1_remelt_D2"]
    L = case["L"]
    lat0 = ic.lattice_of(case)
    calls = bm.calls_of(dict(case, batches=(25, 40)))
    t = bm.table_of(dict(case, batches=(25, 40)))
    lat = oracle_mod.Lattice(*lat0, impurity_c=0.1)
    st = beam_ref.Stepper(lat, t, case["n_sub"], case["threshold"], bc=case["bc"])
    e, e2 = _beam_engine(case, lat0, t), _beam_engine(case, lat0, t)
    sh = dict(SHIFT_A, fill_T=3100.0)
    try:
        for c, call in enumerate(calls):
            if c == 1:
                assert e.shift(**sh) == dict(shift_oracle(lat, **sh), calls=1)
                shift_by_host(e2, **sh)
            ro = st.run_steps(call[0], call[1], case["defect_fraction"], call[2], call[3], call[4], rng_mode=case["rng_mode"], seed=case["seed"],
                              thermal_mode=2, q_planes=None, use_latent=case["use_latent"])
            rg, rg2 = _beam_call(e, case, call), _beam_call(e2, case, call)
            assert ro["status"] == 0 and (c == 0 or events_in_zone(L, sh["d"], ro["events"]) >= 1)
            assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"call {c}")
            assert_twins_agree(rg, rg2, e, e2, f"call {c}")
        assert e.remelt_info()["n_melted"] == st.info["n_melted"] and e.remelt_info() == e2.remelt_info()
    finally:
        e.close()
        e2.close()


def test_shift_behind_a_termination(oracle_mod):
    """a lattice of defects holds no event: status 1 at once.  A recoated layer of empty voxels gives it events again."""
    L = 16
    state = np.full((L, L, L), 4, np.int64)
    z = np.zeros((L, L, L))
    T = np.full((L, L, L), 3000.0)
    lat = (state, z, z, T, np.zeros_like(state))
    e, e2 = _engines(L, lat)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C)
    try:
        (s0, n, up, ud, unp), (s1, n1, up1, ud1, unp1) = batch_calls((30, 40))
        kw = dict(rng_mode=1, seed=1, thermal_mode=1)
        rg, ro = e.run_steps(s0, n, 0.0, up, None, unp, **kw), o.run_steps(s0, n, 0.0, up, None, unp, **kw)
        e2.run_steps(s0, n, 0.0, up, None, unp, **kw)
        assert (ro["done"], ro["status"]) == (0, 1)
        assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, "terminated")
        info = e.shift(**SHIFT_A)
        assert info == dict(shift_oracle(o, **SHIFT_A), calls=1) and info["dropped"] == [0, 0, 0, 0, 4 * L * L, 0]
        shift_by_host(e2, **SHIFT_A)
        rg, ro = e.run_steps(s0, n1, 0.0, up1, None, unp1, **kw), o.run_steps(s0, n1, 0.0, up1, None, unp1, **kw)
        assert (ro["done"], ro["status"]) == (n1, 0) and events_in_zone(L, SHIFT_A["d"], ro["events"]) >= 1
        assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, "behind the shift")
        assert_twins_agree(rg, e2.run_steps(s0, n1, 0.0, up1, None, unp1, **kw), e, e2, "behind the shift")
    finally:
        e.close()
        e2.close()


def test_staged_batch_consumed_behind_a_shift(oracle_mod):
    """the staged batch holds inputs only: a shift between stage_inputs and run_steps leaves it valid, and the batch steps the
    shifted lattice"""
    L = 16
    lat = random_lattice(L, 8)
    e, e2 = _engines(L, lat, FOUR_KIND_PARAMS)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    try:
        (s0, n, up, ud, unp), = batch_calls((40,))
        kw = dict(rng_mode=1, seed=3, thermal_mode=1)
        e.stage_inputs(s0, n, DEFECT_FRACTION, up, ud, unp, **kw)
        h2d = e.counters()["bytes_h2d"]
        assert e.shift(**SHIFT_B) == dict(shift_oracle(o, **SHIFT_B), calls=1)
        shift_by_host(e2, **SHIFT_B)
        rg = e.run_steps(s0, n, DEFECT_FRACTION, up, ud, unp, staged=True, **kw)
        assert e.counters()["bytes_h2d"] == h2d              # neither the shift nor the staged call copied an input
        ro = o.run_steps(s0, n, DEFECT_FRACTION, up, ud, unp, **kw)
        assert (ro["done"], ro["status"]) == (n, 0) and events_in_zone(L, SHIFT_B["d"], ro["events"]) >= 1
        assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, "staged")
        assert_twins_agree(rg, e2.run_steps(s0, n, DEFECT_FRACTION, up, ud, unp, **kw), e, e2, "staged")
    finally:
        e.close()
        e2.close()
