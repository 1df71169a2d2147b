"""The solidification map behind real stepping, against the comparator (solid_ref.py) fed with the ORACLE's state and T after
every call: cetkmc_run_steps in 20-step calls with the temperature update of thermal_mode 1, an update of the map between
the calls.  The map ==, and every voxel stamped by an update is the site an event of that call's log filled (pos of a
deposition, nucleation or attachment, target of a diffusion).  One Mode B case, one on the deferring path (L = 136), and the
proof that the updates perturb nothing: a run with updates between its calls (a staged batch waiting across each) returns the
bits of the same run without."""
import os

import numpy as np
import pytest

import solid_ref as SR
from helpers import (FOUR_KIND_PARAMS, assert_call_matches_oracle, assert_supersteps_match_oracle, batch_calls, oracle_lattice,
                     random_lattice)
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
INV_DX = 2.0e5
THERMAL_DT = 1e-6


def _engine(L, lat):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.upload(*lat)
    return e


def _filled_sites(events):
    """the sites the executed events of a log filled"""
    ev = events.reshape(-1)
    ev = ev[ev["type"] >= 0]
    return {tuple(int(x) for x in (r["target"] if r["type"] == 1 else r["pos"])) for r in ev}


def _check_update(e, ref, lat, events, stamp, tag):
    info = e.solid_update(stamp, THERMAL_DT, INV_DX)
    want = ref.update(lat.state, lat.T, stamp, INV_DX, THERMAL_DT)
    assert info == want, (tag, info, want)
    assert SR.same_map(e.solid_read(), ref.map()) == [], tag
    stamped = {tuple(int(x) for x in v) for v in np.argwhere(ref.stamp == stamp)}
    assert stamped <= _filled_sites(events), (tag, sorted(stamped - _filled_sites(events))[:4])
    return want


@pytest.mark.parametrize("L,n_calls", [(16, 3), (40, 3), (136, 2)])
def test_run_steps_vs_oracle(oracle_mod, L, n_calls):
    """L = 136 is on the deferring path (cetkmc_counters.deferred_steps proves it): the update reads the lattice behind the
    call's last, immediate step"""
    lat = random_lattice(L, 31 + L)
    e = _engine(L, lat)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        e.solid_begin()
        ref = SR.SolidRef(o.state, o.T)
        tot = dict(n_new=0, n_cleared=0)
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(batch_calls((20,) * n_calls)):
            kw = dict(rng_mode=1, seed=5, thermal_mode=1, thermal_dt=THERMAL_DT)
            rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            assert (ro["done"], ro["status"]) == (n, 0)
            want = _check_update(e, ref, o, ro["events"], step0 + n, f"L={L} call {c}")
            # the comparison of the whole call AFTER the update: the update left fields, rate table and lists as they were
            assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"L={L} call {c}")
            for k in tot:
                tot[k] += want[k]
        print(f"L={L}: {tot} recorded {want['n_recorded']}")
        assert tot["n_new"] >= 10 and tot["n_cleared"] >= 1, tot
        assert (e.counters()["deferred_steps"] > 0) == (L > 128)
    finally:
        oracle_mod.set_threads(1)
        e.close()


def test_mode_b_vs_oracle(oracle_mod):
    L, box = 16, 8
    lat = random_lattice(L, 77)
    e = _engine(L, lat)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    try:
        e.solid_begin()
        ref = SR.SolidRef(o.state, o.T)
        n_new = 0
        for c in range(2):
            kw = dict(thermal_mode=1, thermal_dt=THERMAL_DT, want_events=True)
            rg = e.run_supersteps(20 * c, 20, box, DEFECT_FRACTION, 9, **kw)
            ro = o.run_supersteps(20 * c, 20, box, DEFECT_FRACTION, 9, **kw)
            assert (ro["done"], ro["status"]) == (20, 0)
            n_new += _check_update(e, ref, o, ro["events"], 20 * c + 20, f"Mode B call {c}")["n_new"]
            assert_supersteps_match_oracle(e, o, rg, ro, RATE_RTOL, tag=f"Mode B call {c}")
        assert n_new >= 40, n_new                          # several events per super-step
    finally:
        e.close()


def test_updates_perturb_nothing():
    """the same three calls on two handles, one with a map updated between the calls while the next call's batch is staged"""
    L = 16
    lat = random_lattice(L, 5)
    calls = batch_calls((20, 20, 20))
    kw = dict(rng_mode=1, seed=5, thermal_mode=1, thermal_dt=THERMAL_DT)
    out = []
    for with_map in (False, True):
        e = _engine(L, lat)
        try:
            if with_map:
                e.solid_begin()
            res, recorded = [], 0
            for step0, n, u_pick, u_def, u_np in calls:
                e.stage_inputs(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                if with_map:
                    recorded = e.solid_update(step0, THERMAL_DT, INV_DX)["n_recorded"]
                    e.solid_profile()
                res.append(e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, staged=True, **kw))
            assert not with_map or recorded > 0
            cnt = e.counters()
            out.append((res, e.download(defects=True), {k: cnt[k] for k in ("steps", "sweeps", "incremental_steps", "thermal_updates",
                                                                            "table_updates", "interface_launches", "deferred_steps")},
                        e.rate_sweep()))
        finally:
            e.close()
    (ra, fa, ca, sa), (rb, fb, cb, sb) = out
    for a, b in zip(ra, rb):
        for k in ("done", "status", "np_used", "q_used", "nucleation_count", "full_sweeps", "min_margin"):
            assert a[k] == b[k], k
        assert a["totals"].tobytes() == b["totals"].tobytes() and a["events"].tobytes() == b["events"].tobytes()
        assert np.array_equal(a["n_events"], b["n_events"])
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert ca == cb and sa == sb
