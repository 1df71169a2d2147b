"""Replica ensembles (cetkmc.Ensemble through the C ABI) against the oracle directly.

test_gpu_ensemble.py compares ensembles with other GPU runs and with reference fixtures through run_kmc_ensemble, at
L <= 30 and R <= 64.  Here every replica has its own oracle.Lattice and is compared with it after EVERY call: stop state,
stream position, nucleation count, totals, the terminating total, dt (rng_mode 2), all five fields (T included) and the
row sums of the lattice the call left -- at rows longer than one wave (L = 65 .. 128), at L = 1, 2, 3, past the 64-replica
block of k_ens_collect, through terminations and unfreezing under temperature updates, with non-finite temperatures in
one replica, at calls that start at any offset modulo 20, and with per-replica calls between ensemble calls.

Comparators: rng_mode 0 is Lattice.run_steps with each replica's own streams; rng_mode 2 is Lattice.run_supersteps with
box == L.  Tolerances: RATE_RTOL for totals, row sums and dt (as test_gpu_mode_b.py compares dt_event); all else exact.
What a run exercised (event kinds, terminations, defect injections) is computed from the ORACLE's logs and asserted, so
the inputs cannot drift into a run that no longer covers what the test is named for."""
import contextlib
import os

import numpy as np
import pytest

from helpers import (FOUR_KIND_PARAMS, assert_ensemble_call_matches_oracle, face_lattice, oracle_lattice, random_lattice,
                     step_uniforms)
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

CALLS = (7, 1, 13, 20, 19)      # back to back from step 0: starts at 0, 7, 8, 1, 1 modulo 20; updates inside a call and at its edge
N_ATOMS = {33: 400, 64: 1500, 65: 1500, 100: 3000, 127: 6000, 128: 6000}


@contextlib.contextmanager
def _oracle_threads(oracle_mod):
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        yield
    finally:
        oracle_mod.set_threads(1)


class _Run:
    """An ensemble and one oracle lattice per replica, stepped call by call and compared after each.  Which replicas are
    frozen is taken from the oracle's results (status 1) -- a frozen replica's oracle lattice is not stepped."""

    def __init__(self, oracle_mod, L, lattices, impurity_c, nu_scale=None, defect_fraction=0.0, tweak=None, rng_mode=0,
                 seeds=None, thermal_mode=1):
        import cetkmc
        self.o, self.L, self.R = oracle_mod, L, len(lattices)
        self.rng_mode, self.thermal_mode, self.tweak = rng_mode, thermal_mode, dict(tweak or {})
        self.df = np.broadcast_to(np.asarray(defect_fraction, np.float64), (self.R,)).copy()
        self.seeds = np.arange(1, self.R + 1) * 7919 if seeds is None else np.asarray(seeds)
        self.params = []
        for r in range(self.R):
            p = cetkmc.default_params(float(impurity_c[r]))
            for k, v in self.tweak.items():
                setattr(p, k, v)
            p.nu_dep *= 1.0 if nu_scale is None else nu_scale[r]
            self.params.append(p)
        self.ens = cetkmc.Ensemble(L, self.params)
        self.lats = [None] * self.R
        self.frozen = set()
        self.logs = []              # per call: (step0, n, [oracle result or None per replica], [u_defect row or None])
        self.n_calls = 0
        for r, lat in enumerate(lattices):
            self.upload(r, lat)

    def upload(self, r, lat):
        """A new lattice into replica r and a fresh oracle lattice for it.  The nucleation count is a running total on the
        handle (cetkmc.h): an upload does not reset it, so the new oracle lattice inherits it.  Unfreezes the replica."""
        st, th, ph, T, df = lat
        self.ens.replica(r).upload(st, th, ph, T, df)
        nuc = self.lats[r].nuc_count if self.lats[r] is not None else 0
        self.lats[r] = oracle_lattice(self.o, lat, self.params[r].impurity_c, self.tweak)
        self.lats[r].params.nu_dep = self.params[r].nu_dep
        self.lats[r].nuc_count = nuc
        self.frozen.discard(r)

    def call(self, step0, n, tag=""):
        L, R, ens, tm = self.L, self.R, self.ens, self.thermal_mode
        live = [r for r in range(R) if r not in self.frozen]
        ros, u_def = [None] * R, [None] * R
        if self.rng_mode == 0:
            stride = max(n * (L * L + 2), 1)
            u = [step_uniforms(1000 * self.n_calls + r, n, stride) for r in range(R)]
            res = ens.run(step0, n, self.df, np.stack([x[0] for x in u]), np.stack([x[1] for x in u]),
                          np.stack([x[2] for x in u]), rng_mode=0, thermal_mode=tm)
            for r in live:
                ros[r] = self.lats[r].run_steps(step0, n, self.df[r], *u[r], rng_mode=0, thermal_mode=tm)
                u_def[r] = u[r][1]
        else:
            res = ens.run(step0, n, self.df, rng_mode=2, seeds=self.seeds, thermal_mode=tm)
            for r in live:
                ros[r] = self.lats[r].run_supersteps(step0, n, L, self.df[r], int(self.seeds[r]), thermal_mode=tm)
                u_def[r] = np.array([self.o.counter_uniform(int(self.seeds[r]), step0 + x, self.o.KEY_DEFECT) for x in range(n)])
        self.n_calls += 1
        self.logs.append((step0, n, ros, u_def))
        assert_ensemble_call_matches_oracle(ens, self.lats, res, ros, RATE_RTOL,
                                            tag=f"{tag} L={L} R={R} call {self.n_calls - 1} (steps {step0}..{step0 + n - 1})")
        self.frozen |= {r for r in live if ros[r]["status"] == 1}
        return res, ros

    def calls(self, batches, step0=0, tag=""):
        for n in batches:
            self.call(step0, n, tag)
            step0 += n
        return step0

    def coverage(self):
        """From the oracle's logs: events of each kind per replica, defect injections per replica, executed steps per
        replica, (call, step of the call) at which a replica terminated."""
        kinds = np.zeros((self.R, 4), np.int64)
        defects, steps, term = np.zeros(self.R, np.int64), np.zeros(self.R, np.int64), {}
        for c, (step0, n, ros, u_def) in enumerate(self.logs):
            for r, ro in enumerate(ros):
                if ro is None:
                    continue
                ev = ro["events"] if self.rng_mode == 0 else ro["events"][:, 0]
                kinds[r] += np.bincount(ev["type"][:ro["done"]], minlength=4)[:4]
                steps[r] += ro["done"]
                if self.df[r] > 0.0:
                    defects[r] += int((u_def[r][:ro["done"]] < self.df[r]).sum())
                if ro["status"] == 1:
                    term[r] = (c, ro["done"])
        return dict(kinds=kinds, defects=defects, steps=steps, terminated=term)

    def close(self):
        self.ens.close()


def _four_kind_lattices(L, R):
    return [face_lattice(L, 17 + L + r, N_ATOMS[L]) for r in range(R)]


@pytest.mark.parametrize("L", [33, 64, 65, 100, 127, 128])
def test_four_kinds_vs_oracle(oracle_mod, L):
    """Rows of up to two waves, the last partial plane group of the temperature march, the 1024-thread sweep with its
    largest LDS: four replicas that differ in lattice, impurity_c, nu_dep and defect fraction, reference streams, calls
    starting and ending at several offsets modulo 20."""
    R, batches = 4, CALLS
    with _oracle_threads(oracle_mod):
        run = _Run(oracle_mod, L, _four_kind_lattices(L, R), impurity_c=[0.1 * r for r in range(R)], nu_scale=[1.0, 10.0, 1.0, 0.1],
                   defect_fraction=[0.05, 0.0, 0.02, 0.05], tweak=FOUR_KIND_PARAMS, rng_mode=0)
        try:
            run.calls(batches)
        finally:
            run.close()
    cov = run.coverage()
    print(f"L={L} four kinds, reference streams (oracle logs): kinds per replica {cov['kinds'].tolist()} "
          f"defect injections {cov['defects'].tolist()}")
    assert not cov["terminated"] and (cov["steps"] == sum(batches)).all(), cov
    assert cov["kinds"].sum(axis=0).min() >= 2, cov             # deposition, diffusion, nucleation, attachment
    assert cov["defects"].sum() >= 1, cov


@pytest.mark.parametrize("L,R,batches", [(33, 4, CALLS), (64, 4, CALLS), (128, 2, (6,))])
def test_counter_mode_vs_supersteps(oracle_mod, L, R, batches):
    """rng_mode 2 against run_supersteps(box == L): totals, dt and fields per replica; distinct seeds, nu_dep, impurity_c.
    The oracle's super-step path (serial window selection) is the slow part: at L = 128 one call of 6 steps."""
    with _oracle_threads(oracle_mod):
        run = _Run(oracle_mod, L, _four_kind_lattices(L, R), impurity_c=[0.1 * r for r in range(R)],
                   nu_scale=[1.0, 10.0, 1.0, 0.1][:R], defect_fraction=[0.05, 0.0, 0.02, 0.05][:R], tweak=FOUR_KIND_PARAMS,
                   rng_mode=2, seeds=[11 + 1000 * r for r in range(R)])
        try:
            run.calls(batches)
        finally:
            run.close()
    cov = run.coverage()
    print(f"L={L} counter mode (oracle logs): kinds per replica {cov['kinds'].tolist()} defect injections {cov['defects'].tolist()}")
    assert not cov["terminated"] and (cov["steps"] == sum(batches)).all(), cov
    assert (cov["kinds"].sum(axis=0) > 0).sum() >= 3, cov       # at least three of the four kinds in the ensemble
    assert cov["defects"].sum() >= 1, cov


def _fill(r, R):
    if R >= 3 and r == 1:
        return 0.0                  # an empty replica
    if R >= 3 and r == 2:
        return 1.0                  # a full one: nothing can happen, it terminates at once
    return 0.05 + 0.1 * ((7 * r) % 9)


@pytest.mark.parametrize("R", [1, 63, 65, 200])
def test_replica_count_across_collect_block(oracle_mod, R):
    """k_ens_collect takes 64 replicas per block and the replica rides in grid y (z for the march): every replica of
    R = 1, 63, 65 and 200 against its own oracle lattice, 45 steps in two calls."""
    L = 8
    with _oracle_threads(oracle_mod):
        run = _Run(oracle_mod, L, [random_lattice(L, 100 + r, fill=_fill(r, R)) for r in range(R)],
                   impurity_c=[0.05 * (r % 5) for r in range(R)], nu_scale=[(1.0, 3.0, 0.5)[r % 3] for r in range(R)],
                   defect_fraction=[0.02 * (r % 3) for r in range(R)], rng_mode=2, seeds=[3 + 17 * r for r in range(R)])
        try:
            run.calls((23, 22))
        finally:
            run.close()
    cov = run.coverage()
    print(f"R={R} L={L} (oracle logs): kinds in the ensemble {cov['kinds'].sum(axis=0).tolist()} steps min/max "
          f"{cov['steps'].min()}/{cov['steps'].max()} terminated {len(cov['terminated'])} replicas")
    assert cov["steps"].max() == 45, cov
    if R >= 3:
        assert cov["terminated"].get(2) == (0, 0), cov          # the full replica
        assert cov["steps"][1] == 45, cov                       # the empty one runs
    assert R <= 64 or (cov["steps"][64:] == 45).all(), cov      # the replicas of the later collect blocks run to the end


def _termination_lattices(L):
    """Replicas 0 and 2 stop before step 20 (nearly full, default parameters); 1 and 3 are sparse and go on."""
    if L == 4:
        early = [random_lattice(4, 1, fill=0.9), random_lattice(4, 2, fill=0.9)]
    else:
        early = [random_lattice(5, 1, fill=0.95), random_lattice(5, 3, fill=0.95)]
    return [early[0], random_lattice(L, 11, fill=0.05), early[1], random_lattice(L, 12, fill=0.0)]


@pytest.mark.parametrize("L,rng_mode", [(4, 0), (5, 0), (4, 2)])
def test_termination_freeze_unfreeze_under_updates(oracle_mod, L, rng_mode):
    """Call A (45 steps): replicas 0 and 2 terminate before step 20 and ride through two pass-through temperature updates;
    their T and every other field stay what the oracle left at termination.  Call B (20 steps, one more update: the
    other flip parity): frozen, status 1, no steps, same fields.  Then a new lattice into replica 0 and call C from an
    offset != 0 modulo 20: the unfrozen replica follows its new oracle lattice, replica 2 stays frozen."""
    with _oracle_threads(oracle_mod):
        run = _Run(oracle_mod, L, _termination_lattices(L), impurity_c=[0.0, 0.1, 0.2, 0.0], defect_fraction=[0.0, 0.05, 0.0, 0.02],
                   rng_mode=rng_mode, seeds=[5, 6, 7, 8])
        try:
            resA, rosA = run.call(0, 45, "A")
            term = run.coverage()["terminated"]
            print(f"L={L} rng_mode={rng_mode} (oracle logs): terminated at (call, step) {term}")
            assert {0, 2} <= set(term), term
            for r in (0, 2):
                assert term[r][0] == 0 and 0 < term[r][1] < 20, term        # ran, then stopped before the in-batch updates
                assert resA["status"][r] == 1 and resA["done"][r] == rosA[r]["done"]
            assert rosA[1]["done"] == 45 or rosA[3]["done"] == 45, (rosA[1]["done"], rosA[3]["done"])
            resB, _ = run.call(45, 20, "B")
            for r in (0, 2):
                assert resB["status"][r] == 1 and resB["done"][r] == 0
            run.upload(0, random_lattice(L, 21, fill=0.1))
            resC, rosC = run.call(65, 25, "C")
            assert rosC[0] is not None and rosC[0]["done"] > 0, rosC[0]
            assert rosC[2] is None and resC["status"][2] == 1 and resC["done"][2] == 0
        finally:
            run.close()
    cov = run.coverage()
    print(f"L={L} rng_mode={rng_mode} (oracle logs): steps {cov['steps'].tolist()} terminated {cov['terminated']} "
          f"kinds {cov['kinds'].tolist()}")


def _poisoned(oracle_mod, lat, overflow):
    """NaN, +inf and -inf temperatures: at an occupied site, at empty sites with attachment events (rates that read the
    value before any scrub) and in the empty bulk.  Every rate is tested with isfinite (kmc_event_rates.py), so those
    alone change which events exist but leave the total finite.  ``overflow`` adds a huge finite temperature above two
    more such empty sites: their largest attachment rates (linear in the vertical gradient) come to 1.5e308 each, finite
    one by one, and the total overflows to +inf -- the non-finite total of the termination branch."""
    st, th, ph, T, df = lat
    T = T.copy()
    L = st.shape[0]
    occ = np.argwhere(st != 0)
    T[tuple(occ[len(occ) // 2])] = np.nan
    ev, _ = oracle_lattice(oracle_mod, lat, 0.0).enumerate()
    att = np.unique(ev["pos"][ev["type"] == 3], axis=0)
    att = [tuple(q) for q in att if 0 < q[2] < L - 2 and st[q[0], q[1], q[2] + 1] == 0][::7]
    assert len(att) >= 5
    T[att[0]], T[att[1]], T[att[2]] = np.nan, np.inf, -np.inf
    T[L // 2, L // 2, L - 2] = np.nan
    T[L - 1, 0, L - 1] = np.inf
    T[0, L - 1, L - 1] = -np.inf
    if overflow:
        for i, j, k in att[3:5]:
            T[i, j, k + 1] = 1e200
            ev, _ = oracle_lattice(oracle_mod, (st, th, ph, T, df), 0.0).enumerate()
            mine = ev[(ev["type"] == 3) & (ev["pos"] == (i, j, k)).all(axis=1)]
            T[i, j, k + 1] = 1e200 * (1.5e308 / mine["rate"].max())
    return st, th, ph, T, df


@pytest.mark.parametrize("step0,batches", [(0, (7, 13, 5)), (5, (15, 10))])
def test_nonfinite_temperatures_isolated(oracle_mod, step0, batches):
    """Replica 1 holds NaN and +-inf temperatures among two clean replicas.  From step 0 the first update scrubs them and a
    finite run follows.  From step 5 there is no scrub for 15 steps and the total overflows: the oracle terminates on the
    non-finite total; the frozen replica then keeps its NaNs through the update at step 20, which must not scrub a
    passed-through field.  Replicas 0 and 2 follow their clean oracles exactly."""
    L, R = 33, 3
    lats = _four_kind_lattices(L, R)
    lats[1] = _poisoned(oracle_mod, lats[1], overflow=step0 != 0)
    with _oracle_threads(oracle_mod):
        run = _Run(oracle_mod, L, lats, impurity_c=[0.0, 0.1, 0.2], defect_fraction=[0.05, 0.05, 0.0], tweak=FOUR_KIND_PARAMS, rng_mode=0)
        try:
            run.calls(batches, step0=step0)
        finally:
            run.close()
    cov = run.coverage()
    first = run.logs[0][2][1]
    print(f"step0={step0} (oracle logs): steps {cov['steps'].tolist()} terminated {cov['terminated']} replica 1's first call: "
          f"done {first['done']} status {first['status']} last total {first['totals'][-1] if len(first['totals']) else None}")
    assert cov["steps"][0] == cov["steps"][2] == sum(batches), cov
    if step0 == 0:
        assert np.isfinite(run.lats[1].T).all() and cov["steps"][1] == sum(batches), cov       # scrubbed, then a finite run
    else:
        assert cov["terminated"].get(1) == (0, 0) and not np.isfinite(first["totals"][0]), cov  # a non-finite total stops it
        assert np.isnan(run.lats[1].T).sum() == 3 and np.isinf(run.lats[1].T).sum() == 4       # ... and its T stays poisoned


@pytest.mark.parametrize("L", [1, 2, 3])
def test_call_edges_and_per_replica_calls(oracle_mod, L):
    """n_steps = 0, one-step calls, and per-replica thermal_cet / set_defects / rate_sweep between ensemble calls (they
    reset the replica's freshness flags) followed by calls from offsets != 0 modulo 20, at the smallest lattices."""
    R = 3
    lattices = [random_lattice(L, 40 + r, fill=(0.0, 0.5, 0.3)[r]) for r in range(R)]
    with _oracle_threads(oracle_mod):
        run = _Run(oracle_mod, L, lattices, impurity_c=[0.0, 0.1, 0.3], nu_scale=[1.0, 0.1, 10.0], defect_fraction=[0.05, 0.0, 0.5],
                   rng_mode=0)
        try:
            res, _ = run.call(0, 0)                             # nothing runs: not even the update of step 0
            assert (res["done"] == 0).all() and (res["status"] == 0).all()
            for r, lat in enumerate(lattices):
                assert np.array_equal(run.lats[r].state, lat[0]) and np.array_equal(run.lats[r].T, lat[3])
            run.call(0, 1)
            run.call(1, 1)
            for r in sorted(run.frozen):                        # (at L = 1 the single site is taken after one event)
                run.upload(r, lattices[r])
            run.ens.replica(0).thermal_cet(1e-6, scrub_nan=True)
            run.lats[0].thermal_cet(dt=1e-6, scrub_nan=True)
            mask = (np.random.RandomState(L).random_sample((L,) * 3) < 0.5).astype(np.int64)
            run.ens.replica(1).set_defects(mask)
            run.lats[1].defects = np.ascontiguousarray(mask, dtype=np.int8)
            total = run.ens.replica(2).rate_sweep()[0]
            want = run.lats[2].sweep()["total"]
            assert abs(total - want) <= RATE_RTOL * abs(want), (total, want)
            before = run.coverage()["steps"].copy()
            run.call(6, 1)
            assert (run.coverage()["steps"] - before).max() == 1      # a replica stepped behind the per-replica calls
            run.call(7, 0)
            run.call(7, 14)                                     # crosses the update at step 20
        finally:
            run.close()
    cov = run.coverage()
    print(f"L={L} call edges (oracle logs): steps {cov['steps'].tolist()} terminated {cov['terminated']} kinds {cov['kinds'].tolist()}")


def _analysis_vs_engine(ens, an, host_clusters=False):
    import cetkmc
    L = ens.L
    e = cetkmc.Engine(L)
    try:
        for r in range(ens.R):
            rep = ens.replica(r)
            f = rep.download()
            e.upload(f["state"], f["theta"], f["phi"], f["T"], np.zeros_like(f["state"]))
            b = e.clusters(0.5, labels=True)
            for k in ("first", "size", "bbox", "labels"):
                assert np.array_equal(an[r]["clusters"][k], b[k]), (r, k)
            assert np.array_equal(an[r]["counts"], e.species_counts()), r
            assert an[r]["nucleation_count"] == rep.nucleation_count(), r
            for u, v in zip(an[r]["gather"], e.gather_species(3)):
                assert np.array_equal(u, v), r
            if host_clusters:
                import utils
                clusters, visited = utils.get_clusters(f["state"], f["theta"], f["phi"], theta_threshold=0.5)
                assert np.array_equal(an[r]["clusters"]["labels"], np.asarray(visited)), r
                assert an[r]["clusters"]["size"].tolist() == [len(c) for c in clusters], r
    finally:
        e.close()


@pytest.mark.parametrize("L,R", [(64, 3), (16, 70)])
def test_batched_analysis_at_size(oracle_mod, L, R):
    """Ensemble.analyze after 40 steps at L = 64 (k_ens_cc_rank scans 256 chunks, thousands of roots per replica) and at
    R = 70 (past one collect block) against the single-Engine calls on the downloaded fields; at L = 16 also against
    utils.get_clusters on the host.  The 40 steps themselves are compared with the oracle like every other call here."""
    if L == 64:
        lattices = _four_kind_lattices(L, R)
    else:
        lattices = [random_lattice(L, 300 + r, fill=0.1 + 0.05 * (r % 8)) for r in range(R)]
    with _oracle_threads(oracle_mod):
        run = _Run(oracle_mod, L, lattices, impurity_c=[0.05 * (r % 4) for r in range(R)], defect_fraction=0.01, rng_mode=0)
        try:
            run.calls((40,))
            an = run.ens.analyze(0.5, species=3, labels=True)
            n_clusters = [len(a["clusters"]["size"]) for a in an]
            print(f"L={L} R={R}: clusters per replica min/max {min(n_clusters)}/{max(n_clusters)}")
            assert L < 64 or min(n_clusters) >= 2000
            _analysis_vs_engine(run.ens, an, host_clusters=L == 16)
            for r in range(R):
                assert an[r]["nucleation_count"] == run.lats[r].nuc_count, r
        finally:
            run.close()
