"""The origin map behind real stepping: words, census and clock == the comparator (origin_ref.py) fed with the ORACLE's event
log of the same call.  Mode A at L = 16 (reference streams and counter uniforms, incremental on and off, both thermal modes,
a call that terminates, a call that runs out of its stream and its continuation), the deferring path at L = 136, Mode B (box
8 with and without null events, the caller asking for no events; box == L), and the proof that a map perturbs nothing: a run
with a map returns the bits of the same run without."""
import os

import numpy as np
import pytest

import origin_ref as OR
from helpers import (FOUR_KIND_PARAMS, assert_call_matches_oracle, assert_supersteps_match_oracle, batch_calls, oracle_lattice,
                     random_lattice)
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05


def _engine(L, lat):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.upload(*lat)
    return e


class _Ref:
    """the comparator's map of one lattice"""

    def __init__(self, L, state0):
        self.L, self.seq = L, 0
        self.words, self.census = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64)
        self.state0 = np.array(state0)

    def absorb(self, events, group=1):
        self.seq = OR.absorb(self.words, self.census, events, self.seq, group, self.L)

    def check(self, e, state, tag):
        assert np.array_equal(e.origin_words(), self.words), tag
        assert np.array_equal(e.origin_census(), self.census), tag
        assert e.origin_seq() == self.seq, tag
        # what needs no comparator (no upload since begin)
        _, code = OR.decode(self.words)
        fill = (code >= 1) & (code <= 4)
        assert (state[fill] != 0).all() and (state[code == 5] == 0).all(), tag
        assert fill[(state != 0) & (self.state0 == 0)].all(), tag


@pytest.mark.parametrize("rng_mode,incremental,thermal_mode", [(0, False, 1), (2, False, 1), (0, True, 2), (2, True, 2), (1, False, 2)])
def test_mode_a_vs_oracle(oracle_mod, rng_mode, incremental, thermal_mode):
    from cetkmc import synthetic
    L = 16
    lat = random_lattice(L, 31)
    e = _engine(L, lat)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    try:
        e.origin_begin()
        ref = _Ref(L, o.state)
        kinds = np.zeros(4, np.int64)
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(batch_calls((20, 60, 37))):
            if rng_mode == 0:
                u_np = np.random.RandomState(c).random_sample(n * (L * L + 2))
            q = synthetic.laser_planes(L, step0, n) if thermal_mode == 2 else None
            kw = dict(rng_mode=rng_mode, seed=5, thermal_mode=thermal_mode, q_planes=q)
            rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, incremental=incremental, **kw)
            if rng_mode == 2:      # all-counter uniforms: the oracle's single-domain super-steps are these steps
                ro = o.run_supersteps(step0, n, L, DEFECT_FRACTION, 5, thermal_mode=thermal_mode, q_planes=q)
                events = ro["events"][:, 0]
            else:
                ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                events = ro["events"]
            assert (ro["done"], ro["status"]) == (n, 0)
            for f in ("type", "pos", "target"):                # the engine took the oracle's trajectory
                assert np.array_equal(rg["events"][f], events[f]), (c, f)
            ref.absorb(events)
            ref.check(e, o.state, f"call {c}")
            if rng_mode != 2:
                assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"call {c}")
            kinds += np.bincount(events["type"], minlength=4)
        assert ref.seq == 117 and (kinds > 0).sum() >= 3 and kinds[1] > 0, kinds      # diffusions among them
        assert (e.counters()["incremental_steps"] > 0) == incremental
    finally:
        e.close()


def test_terminating_call(oracle_mod):
    """status 1 in the middle of a call: the executed steps are absorbed, the terminating step's slot is not"""
    import cetkmc
    L, n = 16, 30
    state = np.full((L, L, L), 4, np.int64)
    state[3, 4, 5] = state[9, 9, 9] = 0
    zeros = np.zeros((L, L, L))
    T = np.full((L, L, L), 3000.0)
    rs = np.random.RandomState(2)
    u_pick, u_np = rs.random_sample(n), rs.random_sample(2 * n + 2)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        e.upload(state, zeros, zeros, T, None)
        lat = oracle_mod.Lattice(state, zeros, zeros, T, None, impurity_c=IMPURITY_C)
        e.origin_begin()
        ref = _Ref(L, state)
        rg = e.run_steps(0, n, 0.0, u_pick, None, u_np, rng_mode=1, seed=1, thermal_mode=1)
        ro = lat.run_steps(0, n, 0.0, u_pick, None, u_np, rng_mode=1, seed=1, thermal_mode=1)
        done = ro["done"]
        assert rg["status"] == ro["status"] == 1 and rg["done"] == done and 1 <= done < n
        ref.absorb(ro["events"])
        ref.check(e, lat.state, "terminated")
        assert ref.seq == done and int(ref.census[:, 2].sum()) == done
        rg = e.run_steps(done, n, 0.0, u_pick, None, u_np, rng_mode=1, seed=1, thermal_mode=1)       # nothing left to do
        assert (rg["done"], rg["status"]) == (0, 1)
        ref.check(e, lat.state, "terminated at once")
    finally:
        e.close()


def test_stream_exhausted_and_continuation(oracle_mod):
    """status 2: the slot of the step that ran out of its stream is not absorbed; the continuation carries the clock on"""
    L, n = 16, 120
    lat = random_lattice(L, 8)
    e = _engine(L, lat)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    try:
        rs = np.random.RandomState(9)
        u_pick, u_def, u_np = rs.random_sample(n), rs.random_sample(n), rs.random_sample(2 * n + 2)
        kw = dict(rng_mode=1, seed=21, thermal_mode=1)
        e.origin_begin()
        ref = _Ref(L, o.state)
        # a stream of five slots: it runs short once two events have drawn their orientations (a probe run on a copy shows
        # that the call holds more of them than that, at least one of them not in its first step)
        probe = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS).run_steps(0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
        drawing = np.flatnonzero(np.isin(probe["events"]["type"], (0, 2)))
        assert probe["done"] == n and len(drawing) >= 2 and 1 <= drawing[1] < n - 2, drawing
        cap = 5
        rg = e.run_steps(0, n, DEFECT_FRACTION, u_pick, u_def, u_np[:cap], **kw)
        ro = o.run_steps(0, n, DEFECT_FRACTION, u_pick, u_def, u_np[:cap], **kw)
        done = ro["done"]
        assert rg["status"] == ro["status"] == 2 and rg["done"] == done and 1 <= done < n
        ref.absorb(ro["events"])
        ref.check(e, o.state, "stopped")
        assert ref.seq == done
        used = ro["np_used"]
        rg = e.run_steps(done, n - done, DEFECT_FRACTION, u_pick[done:], u_def[done:], u_np[used:], **kw)
        ro = o.run_steps(done, n - done, DEFECT_FRACTION, u_pick[done:], u_def[done:], u_np[used:], **kw)
        assert (ro["done"], ro["status"]) == (n - done, 0)
        ref.absorb(ro["events"])
        ref.check(e, o.state, "continued")
        assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag="continued")
        assert ref.seq == n
    finally:
        e.close()


def test_deferred_path_vs_oracle(oracle_mod):
    """L = 136: most steps launch their selection alone and the next sweep launch applies the event (deferred_steps > 0);
    the log is written there too"""
    L = 136
    lat = random_lattice(L, 31 + L)
    e = _engine(L, lat)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        e.origin_begin()
        ref = _Ref(L, o.state)
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(batch_calls((13, 20))):
            kw = dict(rng_mode=1, seed=5, thermal_mode=1)
            rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            assert (ro["done"], ro["status"]) == (n, 0)
            ref.absorb(ro["events"])
            ref.check(e, o.state, f"L={L} call {c}")
            assert np.array_equal(rg["events"]["pos"], ro["events"]["pos"]) and np.array_equal(rg["events"]["type"], ro["events"]["type"])
        assert e.counters()["deferred_steps"] > 0 and ref.seq == 33
    finally:
        oracle_mod.set_threads(1)
        e.close()


@pytest.mark.parametrize("box,null_events,want_events", [(8, False, False), (8, True, False), (8, True, True), (16, False, False)])
def test_mode_b_vs_oracle(oracle_mod, box, null_events, want_events):
    """every record of super-step t under the ordinal seq + t; the engine keeps the log on the device when the caller asks
    for no events; box == L is a Mode A step per super-step"""
    L = 16
    lat = random_lattice(L, 77)
    e = _engine(L, lat)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    try:
        e.origin_begin()
        ref = _Ref(L, o.state)
        n_ev = n_null = 0
        for c in range(2):
            kw = dict(thermal_mode=1, null_events=null_events)
            rg = e.run_supersteps(20 * c, 20, box, DEFECT_FRACTION, 9, want_events=want_events, **kw)
            ro = o.run_supersteps(20 * c, 20, box, DEFECT_FRACTION, 9, want_events=True, **kw)
            assert (ro["done"], ro["status"]) == (20, 0) and rg["done"] == 20
            D = (L // box) ** 3
            assert ro["events"].shape == (20, D)
            ref.absorb(ro["events"], D)
            ref.check(e, o.state, f"box {box} call {c}")
            n_ev += int((ro["events"]["type"] >= 0).sum())
            n_null += int((ro["events"]["type"] == -2).sum())
            if want_events:
                assert_supersteps_match_oracle(e, o, rg, ro, RATE_RTOL, tag=f"box {box} call {c}")
        assert ref.seq == 40 and n_ev >= 40 and (n_null > 0) == (null_events and box < L), (n_ev, n_null)
    finally:
        e.close()


def test_a_map_perturbs_nothing():
    """the same calls on two handles, one with a map (profiled between the calls while the next call's batch is staged):
    results, event logs, fields, counters and the final sweep are the same bits"""
    L = 16
    lat = random_lattice(L, 5)
    calls = batch_calls((20, 20, 20))
    kw = dict(rng_mode=1, seed=5, thermal_mode=1)
    out = []
    for with_map in (False, True):
        e = _engine(L, lat)
        try:
            if with_map:
                e.origin_begin()
            res = []
            for step0, n, u_pick, u_def, u_np in calls:
                e.stage_inputs(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                if with_map:
                    e.origin_profile()
                    e.origin_census()
                    e.origin_read()
                res.append(e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, staged=True, **kw))
            sup = e.run_supersteps(60, 8, 8, DEFECT_FRACTION, 3, want_events=True)
            assert not with_map or e.origin_seq() == 68
            cnt = e.counters()
            out.append((res, sup, e.download(defects=True), {k: cnt[k] for k in ("steps", "sweeps", "incremental_steps", "thermal_updates",
                                                                                 "table_updates", "interface_launches", "deferred_steps",
                                                                                 "supersteps")},
                        e.rate_sweep(), e.nucleation_count()))
        finally:
            e.close()
    (ra, pa, fa, ca, sa, na), (rb, pb, fb, cb, sb, nb) = out
    for a, b in zip(ra, rb):
        for k in ("done", "status", "np_used", "q_used", "nucleation_count", "full_sweeps", "min_margin"):
            assert a[k] == b[k], k
        assert a["totals"].tobytes() == b["totals"].tobytes() and a["events"].tobytes() == b["events"].tobytes()
        assert np.array_equal(a["n_events"], b["n_events"])
    assert pa["events"].tobytes() == pb["events"].tobytes() and pa["totals"].tobytes() == pb["totals"].tobytes()
    assert np.array_equal(pa["n_exec"], pb["n_exec"])
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert ca == cb and sa == sb and na == nb
