"""Replica ensembles in the laser thermal mode (cetkmc_ens_args.thermal_mode 2) against the oracle.

As in test_gpu_ensemble_vs_oracle.py every replica has its own oracle.Lattice and is compared with it after EVERY call
(stop state, stream position, nucleation count, totals, the terminating total, dt in rng_mode 2, all five fields, row
sums), and in addition q_used after every call and prev_state at the end of a run: one further latent-heat update with a
zero source plane on the replica and on its oracle lattice gives the same T only if the device's prev_state (and the row
flags that say where it may differ from state) are the oracle's.

Comparators: rng_mode 0 is Lattice.run_steps(thermal_mode=2, q_planes=), rng_mode 2 is Lattice.run_supersteps(box=L,
thermal_mode=2, q_planes=); use_latent=0, which the oracle does not have, is compared bit for bit with single cetkmc.Engine
runs.  Tolerances: RATE_RTOL for totals, row sums and dt; everything else exact.  What a run exercised is taken from the
ORACLE's results and asserted."""
import numpy as np
import pytest

from helpers import assert_fields_match_oracle, oracle_lattice, random_lattice, relerr, step_uniforms
from test_gpu_ensemble_vs_oracle import _Run, _oracle_threads
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

DT = 1e-6
# back to back from step 0; three updates each in A (0, 20, 40), B (60, 80, 100) and D (120, 140, 160), none in C (110..118);
# B, C and D start at offsets that are no multiples of 20
CALLS = ((0, 45), (45, 65), (110, 9), (119, 50))
T_HOT0 = 3000.0         # uniform initial temperature of the "hot" lattice: its Laplacian is exactly zero until the pulse
HOT_UPDATE = 1          # the pulse comes with the update of step 20: the hot replica stops in the middle of call A


def hot_pulse_power(o, radius):
    """Power of a defocused pulse (beam radius ``radius`` >> the lattice: uniform over the plane to ~1e-7 relative) that
    lifts a top plane at T_HOT0 in ONE update to the temperature at which a single deposition rate is 1.2e308: finite,
    so every empty top site is a candidate (kmc_event_rates.py:63), while two of them already sum to +inf -- the
    non-finite total of the termination branch (kmc_simulation.py:260).  The window is [~1e308 / sites, 1.797e308] in
    the rate, ~ +-0.14 K in T, against an error of the pulse of ~1e-4 K."""
    x = np.log(1.2e308 / o.NU_DEP)                     # rate = nu_dep * exp((T - T_melt) / (kT * T))
    T_star = o.T_MELT / (1.0 - x * o.K_T)
    q = (T_star - T_HOT0) * (o.RHO * o.CP) / DT        # volumetric source that adds T_star - T_HOT0 in one update
    return q * o.VOXEL_SIZE * np.pi * radius * radius / 0.35


def scan_planes(o, L, scan, step0, n):
    """Source planes (n_updates, L, L) of the updates in [step0, step0 + n): the beam of ``scan`` (power, start, speed,
    optional radius) at start + speed * u for update u = g // 20; ``pulse`` = (u, power, radius) replaces one update."""
    us = [g // 20 for g in range(step0, step0 + n) if g % 20 == 0]
    out = np.zeros((len(us), L, L))
    for x, u in enumerate(us):
        power, radius = scan["power"], scan.get("radius", 50e-6)
        if scan.get("pulse") and scan["pulse"][0] == u:
            _, power, radius = scan["pulse"]
        c = scan["start"] + scan["speed"] * u
        out[x] = o.laser_source_plane(L, (c, c), power, beam_radius=radius)
    return out


def make_scans(L, n):
    """n different scans: power 60 .. 300 W, different start points and speeds (one scans backwards)."""
    return [dict(power=60.0 + 47.0 * (s % 6), start=(0.31 * s * L) % max(L, 1), speed=(0.7, -0.4, 1.3, 0.0)[s % 4]) for s in range(n)]


def hot_lattice(L, seed):
    st, th, ph, T, df = random_lattice(L, seed, fill=0.1)
    st[L - 1, :2, :] = 0                               # empty top sites: the candidates whose rates overflow the sum
    th[L - 1, :2, :] = 0.0
    ph[L - 1, :2, :] = 0.0
    return st, th, ph, np.full_like(T, T_HOT0), df * (st == 3)


def hot_scan(o):
    return dict(power=0.0, start=0.0, speed=0.0, pulse=(HOT_UPDATE, hot_pulse_power(o, 1.0), 1.0))


class _LaserRun(_Run):
    """_Run in thermal_mode 2: ``scans`` are the plane sets of the ensemble, ``q_set`` maps replicas to them (None: set r
    for replica r).  q_used is compared after every call."""

    def __init__(self, oracle_mod, L, lattices, scans, q_set=None, use_latent=True, **kw):
        super().__init__(oracle_mod, L, lattices, thermal_mode=2, **kw)
        self.scans, self.use_latent = scans, use_latent
        self.q_set = None if q_set is None else np.asarray(q_set, np.int32)

    def set_of(self, r):
        return r if self.q_set is None else int(self.q_set[r])

    def call(self, step0, n, tag=""):
        L, R, ens = self.L, self.R, self.ens
        sets = [scan_planes(self.o, L, sc, step0, n) for sc in self.scans]
        n_u = len(sets[0])
        kw = dict(thermal_mode=2, q_planes=np.stack(sets) if n_u else None, q_set=self.q_set, use_latent=self.use_latent)
        live = [r for r in range(R) if r not in self.frozen]
        ros, u_def = [None] * R, [None] * R
        if self.rng_mode == 0:
            stride = max(n * (L * L + 2), 1)
            u = [step_uniforms(1000 * self.n_calls + r, n, stride) for r in range(R)]
            res = ens.run(step0, n, self.df, np.stack([x[0] for x in u]), np.stack([x[1] for x in u]),
                          np.stack([x[2] for x in u]), rng_mode=0, **kw)
            for r in live:
                ros[r] = self.lats[r].run_steps(step0, n, self.df[r], *u[r], rng_mode=0, thermal_mode=2,
                                                q_planes=sets[self.set_of(r)] if n_u else None)
                u_def[r] = u[r][1]
        else:
            res = ens.run(step0, n, self.df, rng_mode=2, seeds=self.seeds, **kw)
            for r in live:
                ros[r] = self.lats[r].run_supersteps(step0, n, L, self.df[r], int(self.seeds[r]), thermal_mode=2,
                                                     q_planes=sets[self.set_of(r)] if n_u else None)
                u_def[r] = np.array([self.o.counter_uniform(int(self.seeds[r]), step0 + x, self.o.KEY_DEFECT) for x in range(n)])
        self.n_calls += 1
        self.logs.append((step0, n, ros, u_def))
        tag = f"{tag} L={L} R={R} call {self.n_calls - 1} (steps {step0}..{step0 + n - 1})"
        from helpers import assert_ensemble_call_matches_oracle
        assert_ensemble_call_matches_oracle(ens, self.lats, res, ros, RATE_RTOL, tag=tag)
        for r in range(R):
            want = 0 if ros[r] is None else ros[r]["q_used"]
            assert int(res["q_used"][r]) == want, (tag, "q_used", r, int(res["q_used"][r]), want)
        self.frozen |= {r for r in live if ros[r]["status"] == 1}
        return res, ros

    def calls(self, batches, tag=""):
        for step0, n in batches:
            self.call(step0, n, tag)

    def check_prev_state(self, replicas=None, tag=""):
        """One latent-heat update with a zero plane on the replica and on its oracle lattice (which keeps its own
        prev_state): equal T <=> the device's prev_state marks the same voxels as solidified since the last update."""
        zero = np.zeros((self.L, self.L))
        for r in range(self.R) if replicas is None else replicas:
            n_new = int(((self.lats[r].prev_state == 0) & (self.lats[r].state != 0)).sum())
            self.ens.replica(r).thermal_laser(DT, zero, use_latent=True, scrub_nan=False)
            self.lats[r].thermal_laser(DT, zero, scrub_nan=False)
            got = self.ens.replica(r).download(state=False, theta=False, phi=False)["T"]
            assert np.array_equal(got, self.lats[r].T, equal_nan=True), (tag, "prev_state (T of a zero-plane latent update)", r,
                                                                       n_new, np.argwhere(got != self.lats[r].T)[:4])


def _lattices(L, R):
    """Random occupation under a smooth temperature ramp along axis 0 (as run_kmc starts from), one offset per replica.
    The reference's update is an explicit Euler step at alpha dt / dx^2 = 2.7: a rough field is at the clip bounds
    everywhere after one update, and there the latent-heat term cannot be seen.  From a ramp the field saturates only
    gradually around the beam and the solidified voxels, so every call's T depends on the term (checked with the oracle,
    latent_coef 0 against the default, when these inputs were chosen)."""
    out = []
    for r in range(R):
        st, th, ph, T, df = random_lattice(L, 500 + 13 * L + r, fill=(0.05, 0.3, 0.15)[r % 3])
        ramp = (2900.0 + 50.0 * (r % 8)) + (600.0 / max(L - 1, 1)) * np.arange(L)
        out.append((st, th, ph, np.repeat(np.repeat(ramp[:, None, None], L, axis=1), L, axis=2), df))
    return out


def _run_kw(R, rng_mode=0):
    return dict(impurity_c=[0.05 * (r % 4) for r in range(R)], nu_scale=[(1.0, 3.0, 0.5)[r % 3] for r in range(R)],
                defect_fraction=[0.02 * (r % 3) for r in range(R)], rng_mode=rng_mode, seeds=[3 + 17 * r for r in range(R)])


@pytest.mark.parametrize("L,R,batches", [(1, 3, CALLS), (2, 3, CALLS), (3, 70, CALLS), (33, 3, CALLS), (64, 3, CALLS), (128, 1, CALLS[:3])])
def test_sizes_vs_oracle(oracle_mod, L, R, batches):
    """Single voxel, the smallest stencils, an odd pitch with partial tiles, 32 plane groups; 1, 3 and 70 replicas, each
    with its own plane set; reference streams; the call without an update passes n_q = 0."""
    with _oracle_threads(oracle_mod):
        run = _LaserRun(oracle_mod, L, _lattices(L, R), make_scans(L, R), **_run_kw(R))
        try:
            run.calls(batches)
            run.check_prev_state(tag=f"L={L} R={R}")
        finally:
            run.close()
    cov = run.coverage()
    q_used = [[0 if ro is None else ro["q_used"] for ro in log[2]] for log in run.logs]
    print(f"L={L} R={R} laser (oracle logs): steps min/max {cov['steps'].min()}/{cov['steps'].max()} terminated "
          f"{len(cov['terminated'])} kinds {cov['kinds'].sum(axis=0).tolist()} q_used per call (replica 0) {[q[0] for q in q_used]}")
    assert [n for _, n in batches][2] < 20 and max(q_used[2]) == 0                 # the call without an update
    if L >= 33:
        assert cov["steps"].max() == sum(n for _, n in batches), cov
        assert max(q_used[0]) == 3 and max(q_used[1]) == 3, q_used


@pytest.mark.parametrize("L,R", [(3, 3), (33, 3)])
def test_counter_mode_vs_supersteps(oracle_mod, L, R):
    """rng_mode 2 against run_supersteps(box == L, thermal_mode=2): totals, dt, q_used and fields per replica."""
    batches = CALLS if L == 3 else CALLS[:3]
    with _oracle_threads(oracle_mod):
        run = _LaserRun(oracle_mod, L, _lattices(L, R), make_scans(L, R), **_run_kw(R, rng_mode=2))
        try:
            run.calls(batches)
            run.check_prev_state(tag=f"counter L={L}")
        finally:
            run.close()
    cov = run.coverage()
    print(f"L={L} R={R} laser, counter mode (oracle logs): steps {cov['steps'].tolist()} terminated {cov['terminated']}")
    assert L < 33 or cov["steps"].max() == sum(n for _, n in batches), cov


def test_shared_plane_sets(oracle_mod):
    """q_set maps seven replicas to three plane sets (the seeds of one map point share a scan)."""
    L, R, q_set = 9, 7, [0, 1, 0, 2, 1, 0, 2]
    with _oracle_threads(oracle_mod):
        run = _LaserRun(oracle_mod, L, _lattices(L, R), make_scans(L, 3), q_set=q_set, **_run_kw(R))
        try:
            run.calls(CALLS)
            run.check_prev_state(tag="shared sets")
        finally:
            run.close()
    cov = run.coverage()
    print(f"shared plane sets (oracle logs): steps {cov['steps'].tolist()} terminated {cov['terminated']}")
    assert cov["steps"].max() == sum(n for _, n in CALLS), cov


def _raw_calls(ens, R, L, row, lat, batches, scans, q_set, use_latent=True):
    """Reference-stream calls on an ensemble whose replica ``row`` holds ``lat`` and draws from streams that depend on the
    call alone; returns what the calls reported for that replica and its final fields."""
    out = []
    for c, (step0, n) in enumerate(batches):
        stride = n * (L * L + 2)
        u = [step_uniforms(7000 + c if r == row else 9000 + 100 * c + r, n, stride) for r in range(R)]
        sets = [scan_planes(_raw_calls.o, L, sc, step0, n) for sc in scans]
        res = ens.run(step0, n, 0.02, np.stack([x[0] for x in u]), np.stack([x[1] for x in u]), np.stack([x[2] for x in u]),
                      rng_mode=0, thermal_mode=2, q_planes=np.stack(sets) if len(sets[0]) else None, q_set=q_set,
                      use_latent=use_latent)
        out.append((int(res["done"][row]), int(res["status"][row]), int(res["np_used"][row]), int(res["q_used"][row]),
                    res["totals"][row].copy()))
    return out, ens.replica(row).download(defects=True)


def test_same_bits_at_index_0_of_1_and_index_37_of_70(oracle_mod):
    """The same lattice, parameters, streams and plane set as the only replica of R = 1 and as replica 37 of R = 70
    (plane set 2 of 4 there): the same results bit for bit."""
    import cetkmc
    _raw_calls.o = oracle_mod
    L, row = 10, 37
    lat = random_lattice(L, 77, fill=0.1)
    scans = make_scans(L, 4)
    results = []
    for R, at, sc, q_set in ((1, 0, [scans[2]], None), (70, row, scans, [2 if r == row else r % 4 for r in range(70)])):
        ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1 if r == at else 0.03 * (r % 5)) for r in range(R)])
        try:
            for r in range(R):
                ens.replica(r).upload(*(lat if r == at else random_lattice(L, 900 + r, fill=0.05 + 0.01 * (r % 20))))
            results.append(_raw_calls(ens, R, L, at, lat, CALLS, sc, q_set))
        finally:
            ens.close()
    (log1, f1), (log70, f70) = results
    for a, b in zip(log1, log70):
        assert a[:4] == b[:4], (a[:4], b[:4])
        assert np.array_equal(a[4], b[4], equal_nan=True)
    assert sum(a[0] for a in log1) == sum(n for _, n in CALLS) and sum(a[3] for a in log1) == 9, log1      # ran, nine planes
    for k in f1:
        assert np.array_equal(f1[k], f70[k], equal_nan=True), k


def test_latent_off_vs_engine_and_latent_matters(oracle_mod):
    """use_latent = 0 (which the oracle does not have) against single cetkmc.Engine runs with use_latent=False, bit for
    bit; and the same ensemble with use_latent = 1 ends with another T in at least one replica -- voxels did solidify
    between two updates, so the latent-heat comparisons of this file are not vacuous."""
    import cetkmc
    _raw_calls.o = oracle_mod
    L, R = 12, 3
    lats, scans = _lattices(L, R), make_scans(L, R)
    batches = CALLS[:2]
    final = {}
    for latent in (False, True):
        for row in range(R):                    # (_raw_calls follows one replica: the streams of ``row`` depend on the call alone)
            ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1) for _ in range(R)])
            try:
                for r in range(R):
                    ens.replica(r).upload(*lats[r])
                final[latent, row] = _raw_calls(ens, R, L, row, lats[row], batches, scans, None, use_latent=latent)
            finally:
                ens.close()
    for row in range(R):
        e = cetkmc.Engine(L, impurity_c=0.1)
        try:
            e.upload(*lats[row])
            log, _ = final[False, row]
            for c, (step0, n) in enumerate(batches):
                u = step_uniforms(7000 + c, n, n * (L * L + 2))
                q = scan_planes(oracle_mod, L, scans[row], step0, n)
                rg = e.run_steps(step0, n, 0.02, *u, rng_mode=0, thermal_mode=2, q_planes=q if len(q) else None, use_latent=False)
                done, status, np_used, q_used, totals = log[c]
                assert (rg["done"], rg["status"], rg["np_used"], rg["q_used"]) == (done, status, np_used, q_used), (row, c)
                if done:
                    assert relerr(totals[:done], rg["totals"][:done]).max() <= RATE_RTOL, (row, c)
            want = e.download(defects=True)
        finally:
            e.close()
        for k in want:
            assert np.array_equal(final[False, row][1][k], want[k], equal_nan=True), (row, k)
    differs = [row for row in range(R) if not np.array_equal(final[False, row][1]["T"], final[True, row][1]["T"])]
    print(f"latent heat changes the final T of replicas {differs}")
    assert differs


def test_termination_freeze_unfreeze(oracle_mod):
    """Replica 1 is the hot one: the defocused pulse of step 20 lifts its whole top plane to deposition rates of ~1e308
    whose sum is +inf, so it stops IN call A (20 steps done, two planes consumed) and rides through the update of step
    40 and call B as a pass-through: T, prev_state and row flags untouched, q_used 0.  A new lattice makes it step again."""
    L, R = 33, 4
    lats = _lattices(L, R)
    lats[1] = hot_lattice(L, 5)
    scans = make_scans(L, R)
    scans[1] = hot_scan(oracle_mod)
    kw = _run_kw(R)
    kw["nu_scale"] = [1.0] * R
    with _oracle_threads(oracle_mod):
        run = _LaserRun(oracle_mod, L, lats, scans, **kw)
        try:
            resA, rosA = run.call(*CALLS[0], tag="A")
            ro = rosA[1]
            print(f"hot replica (oracle): done {ro['done']} status {ro['status']} terminating total {ro['totals'][-1]} q_used {ro['q_used']}; "
                  f"steps of the others {[rosA[r]['done'] for r in (0, 2, 3)]}")
            assert (ro["done"], ro["status"], ro["q_used"]) == (20 * HOT_UPDATE, 1, HOT_UPDATE + 1), ro
            assert not np.isfinite(ro["totals"][ro["done"]]), ro["totals"]
            assert sum(rosA[r]["done"] == CALLS[0][1] for r in range(R)) * 2 >= R, [x["done"] for x in rosA]
            assert int(resA["q_used"][1]) == HOT_UPDATE + 1 and (resA["q_used"][[0, 2, 3]] == 3).all(), resA["q_used"]
            # the update of step 20 (the step it stopped in) left the frozen replica's prev_state level with state, so a
            # pass-through that wrongly synchronised it would not show: give it a prev_state that differs everywhere (this
            # also raises every row flag), on the replica and on its oracle lattice
            run.ens.replica(1).set_prev_state(np.zeros((L,) * 3, np.int64))
            run.lats[1].prev_state = np.zeros((L,) * 3, np.int8)
            resB, rosB = run.call(*CALLS[1], tag="B")
            assert rosB[1] is None and (int(resB["done"][1]), int(resB["status"][1]), int(resB["q_used"][1])) == (0, 1, 0)
            # three more pass-through updates must have left prev_state and the row flags alone: the zero-plane update
            # now adds latent heat at every occupied voxel of the frozen replica, as the oracle's does
            assert (run.lats[1].state != 0).sum() > 100
            run.check_prev_state([1], tag="frozen")
            run.upload(1, random_lattice(L, 31, fill=0.1))
            resC, rosC = run.call(*CALLS[2], tag="C")
            resD, rosD = run.call(*CALLS[3], tag="D")
            assert rosD[1] is not None and rosD[1]["done"] == CALLS[3][1] and int(resD["q_used"][1]) == 3, rosD[1]
            run.check_prev_state(tag="end")
        finally:
            run.close()


def test_per_replica_calls_between_ensemble_calls(oracle_mod):
    """cetkmc_thermal_laser and cetkmc_set_prev_state (an array, and NULL = "level with state") on replica handles
    between two ensemble calls, mirrored on the oracle lattices."""
    L, R = 9, 3
    with _oracle_threads(oracle_mod):
        run = _LaserRun(oracle_mod, L, _lattices(L, R), make_scans(L, R), **_run_kw(R))
        try:
            run.call(0, 33, tag="before")            # ends 13 steps behind an update: prev_state != state
            assert all(((lat.prev_state == 0) & (lat.state != 0)).any() for lat in run.lats)
            plane = oracle_mod.laser_source_plane(L, (4.0, 4.0), 90.0)
            run.ens.replica(0).thermal_laser(DT, plane, use_latent=True, scrub_nan=False)
            run.lats[0].thermal_laser(DT, plane, scrub_nan=False)
            prev = (np.random.RandomState(3).random_sample((L,) * 3) < 0.5) * run.lats[1].state.astype(np.int64)
            run.ens.replica(1).set_prev_state(prev)
            run.lats[1].prev_state = np.ascontiguousarray(prev, dtype=np.int8)
            run.ens.replica(2).set_prev_state(None)
            run.lats[2].prev_state = run.lats[2].state.copy()
            for r in range(R):
                assert_fields_match_oracle(run.ens.replica(r), run.lats[r], RATE_RTOL, f"after the per-replica call, replica {r}")
            run.call(33, 50, tag="after")            # updates at 40, 60, 80
            run.check_prev_state(tag="per-replica calls")
        finally:
            run.close()
    cov = run.coverage()
    print(f"per-replica calls (oracle logs): steps {cov['steps'].tolist()} terminated {cov['terminated']}")
    assert cov["steps"].max() == 83, cov


def test_bad_plane_arguments_are_errors(oracle_mod):
    """n_q too small, q_planes missing with an update due, q_set out of range, n_sets != R with q_set NULL: a non-zero
    return with a message, nothing launched -- every replica is what it was, and the next valid call matches the oracle."""
    L, R = 6, 3
    with _oracle_threads(oracle_mod):
        run = _LaserRun(oracle_mod, L, _lattices(L, R), make_scans(L, R), **_run_kw(R, rng_mode=2))
        try:
            run.call(0, 30, tag="before")
            before = [run.ens.replica(r).download(defects=True) for r in range(R)]
            q3 = np.stack([scan_planes(oracle_mod, L, sc, 30, 50) for sc in run.scans])        # updates at 40, 60 -> (3, 2, L, L)
            assert q3.shape[:2] == (R, 2)
            bad = [("n_q too small", dict(q_planes=q3[:, :1])),
                   ("n_q too small", dict(q_planes=None)),                       # (the binding passes n_q = 0 with no planes)
                   ("q_set", dict(q_planes=q3, q_set=[0, 3, 1])),
                   ("q_set", dict(q_planes=q3, q_set=[0, -1, 1])),
                   ("n_sets must equal R", dict(q_planes=q3[:2])),
                   ("n_sets must equal R", dict(q_planes=np.concatenate([q3, q3[:1]])))]
            for what, kw in bad:
                with pytest.raises(RuntimeError, match=what):
                    run.ens.run(30, 50, run.df, rng_mode=2, seeds=run.seeds, thermal_mode=2, **kw)
                for r in range(R):
                    now = run.ens.replica(r).download(defects=True)
                    for k in now:
                        assert np.array_equal(now[k], before[r][k], equal_nan=True), (what, r, k)
            # q_planes NULL although n_q covers the updates: only the C ABI can say that
            import ctypes as C
            from cetkmc import _lib
            a = _lib.EnsArgs()
            sd = np.ascontiguousarray(run.seeds, dtype=np.uint64)
            a.step0, a.n_steps, a.defect_fraction = 30, 50, run.df.ctypes.data_as(C.POINTER(C.c_double))
            a.seed, a.rng_mode, a.thermal_mode, a.thermal_dt = sd.ctypes.data_as(C.POINTER(C.c_uint64)), 2, 2, DT
            a.q_planes, a.n_q, a.n_sets, a.q_set, a.use_latent = None, 2, R, None, 1
            res = (_lib.RunResult * R)()
            assert run.ens.lib.cetkmc_run_ensemble(run.ens.h, C.byref(a), res, None, None) != 0
            assert "q_planes" in run.ens.error() and "required" in run.ens.error(), run.ens.error()
            for r in range(R):
                now = run.ens.replica(r).download(defects=True)
                for k in now:
                    assert np.array_equal(now[k], before[r][k], equal_nan=True), ("q_planes NULL", r, k)
            run.call(30, 50, tag="after the refused calls")
            run.check_prev_state(tag="errors")
        finally:
            run.close()
