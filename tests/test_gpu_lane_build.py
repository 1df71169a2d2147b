"""Option lane_build: the temperature tiles that write the rate table (k_thermal_tiles16<.., TABLE, LANES>, L = 256) store the
lane table of the entries they write, against the plain sweep that builds it behind the update (lane_build 0), and each against
the oracle.  Option lane_sweep rides along: with it (default) the plain launch on a fresh lane table reads lane sums.

The tiles store a node and a count for EVERY chunk without reading a class byte; the building sweep stores them for pristine
chunks only and poisons the others.  The two tables therefore differ on chunks that hold an atom, and must agree on every chunk
of 8 empty voxels: there a count says "pristine and no entry written since", which the consumer (lane_request()) relies on.

L = 256 is the only shape here at which the fused temperature tiles run.  The lattice is test_gpu_fused_tiles': a solid base
k < 64, the interface sheet behind it, 24000 strewn atoms."""
import os

import numpy as np
import pytest

from helpers import (FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, face_lattice, oracle_lattice, step_uniforms)
from test_gpu_lane_sums import ramp_lattice, uniform_lattice
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

L = 256
IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
N_ATOMS = 24000
POISON = 0xFF


def _engine(lat, tweak, lane_build=1, lane_sweep=1, remelt=None):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in tweak.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.set_option("lane_build", lane_build)
    e.set_option("lane_sweep", lane_sweep)
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


def _observed(e, r):
    d = e.download(defects=True)
    return (r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["full_sweeps"], r["totals"].tobytes(),
            r["events"].tobytes(), r["n_events"].tobytes()) + tuple(d[k].tobytes() for k in sorted(d))


@pytest.fixture
def threads(oracle_mod):
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    yield
    oracle_mod.set_threads(1)


def _one_update_step(lat, tweak):
    """one call of one update step on two engines; their lane tables and the state behind it"""
    from cetkmc import synthetic
    u_pick, u_def, u_np = step_uniforms(100, 1, 4)
    kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, 0, 1))
    out = {}
    for lb in (1, 0):
        e = _engine(lat, tweak, lane_build=lb)
        r = e.run_steps(0, 1, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
        assert (r["done"], r["status"]) == (1, 0)
        t = e.lane_table()
        # the update's tiles built and the plain launch behind it did not, or the reverse
        assert (t["builds_thermal"], t["builds"]) == ((1, 0) if lb else (0, 1)), (lb, t)
        assert t["fresh"] == 1 and t["chunks"] == L * L * (L // 8), (lb, t)
        sums, counts = e.lane_table_arrays()
        out[lb] = (sums, counts, e.download()["state"], t)
        e.close()
    assert np.array_equal(out[1][2], out[0][2])
    return out


def _compare_empty_chunks(out):
    (s1, c1, state, t1), (s0, c0, _, t0) = out[1], out[0]
    empty = (state.reshape(L, L, L // 8, 8) == 0).all(axis=3)
    assert np.array_equal(c1[empty], c0[empty]), ("count bytes of chunks of 8 empty voxels differ", int((c1[empty] != c0[empty]).sum()),
                                                   np.argwhere(empty & (c1 != c0))[:4])
    counted = empty & (c0 <= 8)
    assert np.array_equal(s1[counted].view(np.int64), s0[counted].view(np.int64)), ("lane sums differ", np.argwhere(counted & (s1.view(np.int64) != s0.view(np.int64)))[:4])
    assert set(np.unique(c0[empty])) <= set(range(9)) | {POISON}
    # the tiles store a count for every chunk; what is poisoned there was poisoned by a later write of an entry
    assert t1["usable"] > t0["usable"] and t1["usable"] + t1["poisoned"] == t1["chunks"]
    n_counted, n_poisoned = int(counted.sum()), int((empty & (c0 == POISON)).sum())
    print(f"chunks {empty.size}: of 8 empty voxels {int(empty.sum())}, compared with a count {n_counted}, as poisoned {n_poisoned}, "
          f"with a count below 8: {int((counted & (c0 < 8)).sum())}; lane_build 1 {t1}; lane_build 0 {t0}")
    return counted, c0, s0, n_counted, n_poisoned, empty


def test_lane_tables_equal_on_empty_chunks_ramp_field():
    """the ramp field: the last voxels of a row have dT <= delta_T_c (no rate), so the row's last chunk counts fewer than 8"""
    counted, c0, s0, n_counted, n_poisoned, empty = _compare_empty_chunks(_one_update_step(face_lattice(L, 17 + L, N_ATOMS), FOUR_KIND_PARAMS))
    assert 2 * n_counted >= empty.size, "at least half of the owned chunks are compared with a count"
    assert n_poisoned >= L * L, "the sheet's empty side: a poisoned chunk per row"
    assert int((counted & (c0 < 8)).sum()) >= 1 and int((counted & (c0 == 8)).sum()) >= 1
    assert (s0[counted & (c0 > 0)] > 0.0).all()


def test_lane_tables_equal_on_empty_chunks_uniform_field():
    """4 K under the melting point: no bulk entry has a rate, every sum is +0.0 and every count 0"""
    counted, c0, s0, n_counted, n_poisoned, empty = _compare_empty_chunks(_one_update_step(uniform_lattice(L), FOUR_KIND_PARAMS))
    assert 2 * n_counted >= empty.size and n_poisoned >= L * L
    assert (c0[counted] == 0).all() and (s0[counted].view(np.int64) == 0).all()


def test_trajectory_25_steps(oracle_mod, threads):
    """25 steps from step 0, updates at 0 and 20: lane_build 1 / 0 and lane_sweep 1 / 0 bit for bit, each against the oracle"""
    from cetkmc import synthetic
    lat = face_lattice(L, 17 + L, N_ATOMS)
    (call,) = batch_calls((25,))
    step0, n, u_pick, u_def, u_np = call
    kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, step0, n))
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
    assert (ro["done"], ro["status"]) == (n, 0)
    seen = {}
    for opt in ((1, 1), (0, 1), (1, 0), (0, 0)):
        e = _engine(lat, FOUR_KIND_PARAMS, *opt)
        rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
        seen[opt] = _observed(e, rg)
        assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"(lane_build, lane_sweep) = {opt}")
        t = e.lane_table()
        assert t["fresh"] == 1 and (t["builds_thermal"], t["builds"]) == ((2, 0) if opt[0] else (0, 2)), (opt, t)
        e.close()
    for opt in ((0, 1), (1, 0), (0, 0)):
        for q, (x, y) in enumerate(zip(seen[(1, 1)], seen[opt])):
            assert x == y, f"item {q} of the observed state differs between (lane_build, lane_sweep) = (1, 1) and {opt}"


def test_stream_runs_out_on_an_update_step(oracle_mod, threads):
    """the call 15..24 runs out of orientation draws ON step 20, behind that step's update (whose tiles built the lane table and
    whose table the stop leaves stale); the continuation from step 20 skips the update and rebuilds with a plain sweep"""
    from cetkmc import synthetic
    lat = ramp_lattice(L)
    s0, n, n2 = 15, 10, 5
    u_pick, u_def, u_np = step_uniforms(321, n + n2, 2 * (n + n2) + 2)
    kw = dict(rng_mode=1, seed=5, thermal_mode=2)
    probe = oracle_lattice(oracle_mod, lat, IMPURITY_C)
    rp = probe.run_steps(s0, 5, DEFECT_FRACTION, u_pick[:5], u_def[:5], u_np, q_planes=np.zeros((0, L, L)), **kw)
    cut = rp["np_used"]
    # step 19 drew two orientations (a deposition or a nucleation), so a stream of `cut` doubles lets it run and leaves step 20 short
    assert rp["done"] == 5 and int(rp["events"]["type"][4]) in (0, 2) and cut >= 2
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C)
    calls = [(s0, n, u_pick[:n], u_def[:n], u_np[:cut]), (20, n2, u_pick[5:5 + n2], u_def[5:5 + n2], u_np[cut:])]
    engines = {lb: _engine(lat, {}, lane_build=lb) for lb in (1, 0)}
    for c, (g0, m, up, ud, unp) in enumerate(calls):
        q = synthetic.laser_planes(L, g0, m)
        if c == 0:
            ro = o.run_steps(g0, m, DEFECT_FRACTION, up, ud, unp, q_planes=q, **kw)
        else:
            # step 20's update is in the oracle's field already (it precedes the selection that found the stream short), and the
            # handle remembers that: the continuation does not repeat it, and counts the plane it is handed again (cetkmc.h)
            ro = o.run_steps(g0, m, DEFECT_FRACTION, up, ud, unp, **dict(kw, thermal_mode=0))
            assert ro["q_used"] == 0
            ro["q_used"] = 1
        assert (ro["done"], ro["status"]) == ((5, 2), (n2, 0))[c], (c, ro["done"], ro["status"])
        seen = {}
        for lb, e in engines.items():
            rg = e.run_steps(g0, m, DEFECT_FRACTION, up, ud, unp, q_planes=q, **kw)
            seen[lb] = _observed(e, rg)
            assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"call {c}, lane_build {lb}")
        for q_, (x, y) in enumerate(zip(seen[1], seen[0])):
            assert x == y, f"call {c}: item {q_} of the observed state differs between lane_build 1 and 0"
    t1, t0 = engines[1].lane_table(), engines[0].lane_table()
    # call 0: the plain launch of step 15 builds (the table is k_rate_table's), the update of step 20 builds in its tiles; behind the
    # stop the table is recomputed and a plain launch builds again.  With the option off every build is a plain launch's
    assert (t1["builds_thermal"], t1["builds"]) == (1, 2) and (t0["builds_thermal"], t0["builds"]) == (0, 3), (t1, t0)
    for e in engines.values():
        e.close()


def test_remelting_behind_the_update_falls_back_to_the_building_sweep(oracle_mod):
    """remelting is on: the melt pass behind every update may write class bytes and list voxels outside the batched apply, so
    the lane table the tiles stored is reported stale and the next plain launch builds, as with the option off"""
    import remelt_cases as rc
    case = rc.STEPPING["L256_fused_tiles"]
    run = rc.stepped("L256_fused_tiles")
    oracle_mod.set_threads(case["threads"])
    import cetkmc
    try:
        for lb in (1, 0):
            e = cetkmc.Engine(L, impurity_c=0.1)
            e.set_option("lane_build", lb)
            e.upload(*run["lat0"])
            e.set_remelt(True, case["threshold"])
            n_upd = 0
            for c, (g0, m, up, ud, unp, q) in enumerate(run["calls"]):
                rg = e.run_steps(g0, m, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"], thermal_mode=2,
                                 q_planes=q, use_latent=case["use_latent"], incremental=case["incremental"])
                assert_call_matches_oracle(e, rc.LatView(run, c, 0.1), rg, run["results"][c], RATE_RTOL, f"call {c}, lane_build {lb}")
                n_upd += sum(1 for g in range(g0, g0 + m) if g % 20 == 0)
            t = e.lane_table()
            assert n_upd >= 2 and e.remelt_info()["n_melted"] > 0
            # the first plain launch (step 19, k_rate_table's table) builds, then one plain launch behind every update
            assert t["builds"] == 1 + n_upd and t["builds_thermal"] == (n_upd if lb else 0) and t["fresh"] == 1, (lb, t, n_upd)
            e.close()
    finally:
        oracle_mod.set_threads(1)
