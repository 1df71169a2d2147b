"""Option lane_sums: the census-free tiles that request one stored sum for a lane of 8 empty, unlisted voxels, against the same
tiles reading the lane's 8 rate-table entries, bit for bit, and each against the oracle.

A chunk is the 8 table entries a sweep lane owns.  The plain sweep that follows a table write stores, per chunk whose 8 class
bytes are all 0x01 (pristine), the node tree8(entries) and the number of non-zero entries; every other chunk gets the count
byte 0xFF, and so does the chunk of every entry ifc_store() writes afterwards.  While that lane table is fresh, a lane of the
deferred launches' tiles whose class word is pristine and whose count byte is a count requests the 8 B sum instead of the
64 B of entries (csrc/kernels.hpp, "lane sums").  Everything a step computes must be what it was.

Every case runs 45 or 46 steps with thermal_mode = 2 on two engines (option 1 and 0) and the oracle: the table is rebuilt behind
every temperature update -- twice inside one call, and once by a call whose first step is an update step (RAMP_BATCHES) -- and
the comparison is made after every call.  Cases: the ramp field at L = 129, 136 and 160 (at L = 136 and 160 the row's last
voxel has dT <= delta_T_c, so its chunk counts 7; nucleations in the bulk are about half of the events: each turns a pristine
chunk into an interface chunk and makes ifc_store() write into its neighbours' chunks; the other half are depositions); a
uniform field above T_melt - delta_T_c (every bulk entry is zero: sum 0, count 0); the lattice of test_gpu_lane_skip with its steered diffusions, its attachments, six wholly solid
rows and a wholly solid plane; and a run with a direct cetkmc_apply, an upload and a parameter change between the calls, each of
which the next call must answer with a rebuild.

So that the comparison cannot pass with the fast path idle, cetkmc_lane_table() is read: right after a build at least half of
the owned chunks hold a count (by geometry 11 of the 17 chunks of a row at L = 129: lanes 0..3 are solid, lane 4 holds the
interface sheet, lane 16 is the padded chunk); after the steps more chunks are poisoned than after that build; the number of
builds is the number of table writes; with the option off nothing is built and the table is never fresh."""
import os

import numpy as np
import pytest

from helpers import FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, count_deferred, deferred_coverage, oracle_lattice
from live_ops import oracle_loop_event
from test_gpu_lane_skip import BATCHES as SKIP_BATCHES, SEED as SKIP_SEED, _observed, lattice as skip_lattice, run_oracle_call, top_diffusions
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
RAMP_BATCHES = (40, 6)             # steps 0..45: updates at steps 0 and 20 inside the first call, at step 40 = the second call's first
MUT_BATCHES = (7, 9, 11, 18)       # steps 0..44, a mutator in front of the second, third and fourth call; updates at 0, 20, 40
N_STREWN = 4000


def n_updates(calls):
    return sum(1 for (step0, n, *_) in calls for g in range(step0, step0 + n) if g % 20 == 0)


def ramp_lattice(L):
    from cetkmc import synthetic
    return synthetic.planes(L, 0, L, seed=17 + L, fill_frac=0.25)


def uniform_lattice(L):
    """a uniform field 4 K under the melting point (dT = 4 <= delta_T_c = 10: no bulk nucleation), atoms strewn into the melt so
    that attachments and diffusions happen away from the sheet as well"""
    from cetkmc import synthetic
    from constants import DELTA_T_C, T_MELT
    assert DELTA_T_C > 4
    st, th, ph, T, df = synthetic.planes(L, 0, L, seed=17 + L, constant_T=T_MELT - 4.0, fill_frac=0.25)
    rs = np.random.RandomState(L)
    idx = rs.randint(0, L, (N_STREWN, 3))
    st[idx[:, 0], idx[:, 1], idx[:, 2]] = rs.randint(1, 4, N_STREWN)
    return st, th, ph, T, df


def _engine(L, lat, on, tweak):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in tweak.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.set_option("lane_sums", on)
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


def _check_off(e, tag):
    t = e.lane_table()
    assert t["fresh"] == 0 and t["builds"] == 0, (tag, "lane_sums 0: no lane sum is built or read", t)


class Case:
    """two engines and the oracle on one lattice; run() makes one stepping call on all three and compares"""

    def __init__(self, oracle_mod, L, lat, tweak):
        self.om, self.L, self.tweak = oracle_mod, L, tweak
        self.o = oracle_lattice(oracle_mod, lat, IMPURITY_C, tweak)
        self.engines = {s: _engine(L, lat, s, tweak) for s in (1, 0)}
        self.ran, self.logs = [], []
        # a plain sweep of the lattice as uploaded: it builds (the table and the interface sums are written in front of it)
        for e in self.engines.values():
            assert e.lane_table()["fresh"] == 0
            e.rate_sweep()
        self.built = self.table("after the first build")
        assert self.built["fresh"] == 1 and self.built["builds"] == 1, self.built
        assert self.built["chunks"] == L * L * ((L + 7) // 8) and self.built["usable"] + self.built["poisoned"] == self.built["chunks"], self.built
        assert 2 * self.built["usable"] >= self.built["chunks"], ("at least half of the owned chunks hold a lane sum", self.built)
        _check_off(self.engines[0], "after the first sweep")

    def table(self, tag):
        t = self.engines[1].lane_table()
        print(f"L={self.L} lane table {tag}: {t}")
        return t

    def run(self, call, kw, ro, tag):
        step0, n, u_pick, u_def, u_np = call
        self.ran.append(call)
        self.logs.append(ro)
        seen = {}
        for s, e in self.engines.items():
            rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            seen[s] = _observed(e, rg)
            assert_call_matches_oracle(e, self.o, rg, ro, RATE_RTOL, tag=f"L={self.L} {tag}, lane_sums {s}")
        for q, (x, y) in enumerate(zip(seen[1], seen[0])):
            assert x == y, f"L={self.L} {tag}: item {q} of the observed state differs between lane_sums 1 and 0"
        assert ro["done"] == n and ro["status"] == 0

    def run_plain(self, call, tag):
        from cetkmc import synthetic
        step0, n, u_pick, u_def, u_np = call
        kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(self.L, step0, n))
        ro = self.o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
        self.run(call, kw, ro, tag)

    def finish(self, extra_builds=0):
        """what the run exercised and what the lane table did; returns the deferred steps' coverage (oracle's log)"""
        end = self.table("after the steps")
        # (every call ends with assert_call_matches_oracle's plain sweep of a lattice whose lane table is still fresh: no build)
        assert end["fresh"] == 1 and end["builds"] == 1 + n_updates(self.ran) + extra_builds, (end, n_updates(self.ran), extra_builds)
        assert end["poisoned"] > self.built["poisoned"], ("the events poisoned no chunk", self.built, end)
        assert 2 * end["usable"] >= end["chunks"], end
        _check_off(self.engines[0], "after the steps")
        n_def = count_deferred(self.ran)
        for e in self.engines.values():
            cnt = e.counters()
            assert cnt["deferred_steps"] == n_def and cnt["incremental_steps"] == 0, cnt
            e.close()
        cov = deferred_coverage(self.L, self.ran, self.logs, DEFECT_FRACTION)
        print(f"L={self.L} deferred-step coverage (oracle log): {cov}")
        return cov


@pytest.fixture
def threads(oracle_mod):
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    yield
    oracle_mod.set_threads(1)


def _ramp(oracle_mod, L, batches):
    c = Case(oracle_mod, L, ramp_lattice(L), {})
    if L == 129:        # lanes 5..15 of every row: empty, unlisted
        assert c.built["usable"] == 11 * L * L, c.built
    for k, call in enumerate(batch_calls(batches)):
        c.run_plain(call, f"call {k}")
    cov = c.finish()
    # (the oracle's log: about half of the events of the ramp lattice are bulk nucleations, the others depositions)
    assert cov["kinds"][2] >= 10, ("bulk nucleations on deferred steps", cov)
    return cov


def test_lane_sums_ramp_L129(oracle_mod, threads):
    """Odd L: the last row pair is half empty, the last chunk of a row is padded (poisoned by the build)."""
    _ramp(oracle_mod, 129, RAMP_BATCHES)


def test_lane_sums_ramp_L136(oracle_mod, threads):
    """k = 135 has dT = 6.6 <= delta_T_c: lane 16 of every row counts 7 non-zero entries."""
    _ramp(oracle_mod, 136, RAMP_BATCHES)


def test_lane_sums_ramp_L160(oracle_mod, threads):
    """20 chunks per row; k = 159 (dT = 5.6) is the voxel without a nucleation rate."""
    _ramp(oracle_mod, 160, RAMP_BATCHES)


def test_lane_sums_uniform_field_L136(oracle_mod, threads):
    """every bulk entry is zero: the lane sums are 0 with count 0, the events are depositions, attachments and diffusions"""
    L = 136
    c = Case(oracle_mod, L, uniform_lattice(L), FOUR_KIND_PARAMS)
    sw = c.o.sweep()
    assert sw["n_events"] > 0
    for k, call in enumerate(batch_calls(RAMP_BATCHES)):
        c.run_plain(call, f"call {k}")
    cov = c.finish()
    assert cov["kinds"][2] == 0 and sum(cov["kinds"]) == count_deferred(c.ran), cov


def test_lane_sums_steered_L136_solid(oracle_mod, threads):
    """test_gpu_lane_skip's lattice (kfill = 34 = L / 4, strewn atoms, six wholly solid rows, the solid plane 71, two lone
    top-layer atoms) and its calls: the first pick of each call is steered to a diffusion of a lone atom; attachments follow
    from the strewn atoms."""
    L = 136
    c = Case(oracle_mod, L, skip_lattice(L, SKIP_SEED[L], True), FOUR_KIND_PARAMS)
    steered = []
    for k, call in enumerate(batch_calls(SKIP_BATCHES)):
        call, kw, ro = run_oracle_call(oracle_mod, c.o, L, k, call, steered)
        c.run(call, kw, ro, f"call {k}")
    cov = c.finish()
    top = top_diffusions(c.ran, c.logs)
    assert set(steered) <= set(top) and len(top) >= 2, (steered, top)
    assert cov["kinds"][1] >= 2 and cov["kinds"][3] >= 1, cov            # the steered diffusions; attachments


def test_lane_sums_rebuild_after_mutators_L129(oracle_mod, threads):
    """a direct cetkmc_apply, an upload of T and a parameter change between calls: each leaves the lane table stale, and the
    next call's first sweep -- a plain launch, no update step -- rebuilds it"""
    L = 129
    c = Case(oracle_mod, L, ramp_lattice(L), FOUR_KIND_PARAMS)
    e1, e0, o = c.engines[1], c.engines[0], c.o
    calls = batch_calls(MUT_BATCHES)
    assert all(call[0] % 20 for call in calls[1:])

    def apply_direct():
        rs = np.random.RandomState(7)
        ev, r, th, ph, mk, sw = oracle_loop_event(o, rs.random_sample(1), np.ones(1), rs.random_sample(2), 0)
        assert ev is not None
        for e in (e1, e0):
            e.rate_sweep()
            g = e.select(r)
            assert (g.type, tuple(g.pos), tuple(g.target)) == (ev.type, tuple(ev.pos), tuple(ev.target))
            g.atom = ev.atom
            e.apply(g, th, ph, False)
        o.apply(ev, th, ph, False)

    def upload_T():
        T = o.T + 3.0 * np.cos(np.arange(L))[None, :, None]
        o.T = T.copy()
        for e in (e1, e0):
            e.upload(T=T)

    def set_params():
        o.params.I0 = 3e11
        for e in (e1, e0):
            e.params.I0 = 3e11
            e.set_params()

    mutators = (None, apply_direct, upload_T, set_params)
    for k, (call, mut) in enumerate(zip(calls, mutators)):
        if mut:
            mut()
            t = e1.lane_table()
            assert t["fresh"] == 0, (mut.__name__, t)
            builds = t["builds"]
        c.run_plain(call, f"call {k}")
        if mut:
            t = e1.lane_table()
            assert t["fresh"] == 1 and t["builds"] == builds + 1 + n_updates([call]), (mut.__name__, t, builds)
    c.finish(extra_builds=3)
