"""Shared test helpers: fixture loading and a run_kmc replay driver.

``replay_run_kmc`` re-enacts kmc_simulation.py:203-398 of the reference with the host
RNG streams (CPython ``random`` + NumPy legacy global) handled exactly as the reference
does, on top of an abstract *backend* offering sweep / select / apply / thermal.  The
same driver is used with the CPU oracle (not-gpu tests) and with the HIP engine (gpu
tests), so both are checked against the same reference-generated trajectories.
"""
import os
import random

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TYPE_NAMES = ("dep", "diff", "nuc", "att")


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)


def relerr(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    den = np.maximum(np.abs(b), 1e-300)
    out = np.abs(a - b) / den
    out[(a == b)] = 0.0
    return out


def fixture_step_diffs(z):
    """step -> {flat_idx: (state, theta, phi)} from a traj fixture."""
    d = {}
    for s, fi, st, th, ph in zip(z["diff_step"], z["diff_idx"], z["diff_state"], z["diff_theta"], z["diff_phi"]):
        d.setdefault(int(s), {})[int(fi)] = (int(st), float(th), float(ph))
    return d


class OracleBackend:
    """Backend protocol over oracle.Lattice (canonical-tree selection, like the GPU)."""

    def __init__(self, oracle_mod, state, theta, phi, T, defects, impurity_c):
        self.o = oracle_mod
        self.lat = oracle_mod.Lattice(state, theta, phi, T, defects, impurity_c=impurity_c)
        self._sw = None

    def thermal_cet(self, dt):
        self.lat.thermal_cet(dt=dt, scrub_nan=True)

    def sweep(self):
        self._sw = self.lat.sweep()
        return self._sw["total"], self._sw["n_events"], self._sw["n_dep"]

    def select(self, r):
        sw = self._sw
        return self.lat.select_tree(sw["blocksum"], sw["blockcnt"], sw["rowsum"], sw["rowcnt"], r)

    def apply(self, ev, theta_new, phi_new, make_defect):
        self.lat.apply(ev, theta_new, phi_new, make_defect)

    def set_defects(self, mask):
        self.lat.defects = np.ascontiguousarray(mask, dtype=np.int8)

    def fields(self):
        return self.lat.state, self.lat.theta, self.lat.phi, self.lat.T


def dep_species(u, impurity_c, impurity_re=0.10):
    """kmc_event_rates.py:66-71"""
    if u < impurity_c:
        return 3
    if u < impurity_c + impurity_re:
        return 2
    return 1


def replay_run_kmc(z, make_backend, check_every_step=True, rate_rtol=1e-12):
    """Re-enact run_kmc (kmc_simulation.py:203-398) on a backend and compare with the
    trajectory fixture ``z`` step by step.  Returns the backend."""
    import defects as host_defects
    import lattice_init as host_init

    L, n_steps = int(z["L"]), int(z["n_steps"])
    temp, df = float(z["temp"]), float(z["defect_fraction"])
    n_seeds, c = int(z["n_seeds"]), float(z["impurity_c"])
    diffs = fixture_step_diffs(z)
    Tsnap = {int(s): t for s, t in zip(z["T_steps"], z["T_snaps"])}
    Dsnap = {int(s): d for s, d in zip(z["D_steps"], z["D_snaps"])}

    np.random.seed(42)
    random.seed(42)
    state, theta, phi, T, atom = host_init.initialize_lattice(lattice_size=L, n_seeds=n_seeds, T_sub=temp, impurity_c=c)
    mask, _ = host_defects.introduce_defects(state, atom, T, apply_to_state=False)
    be = make_backend(state, theta, phi, T, mask, c)
    total_time = 0.0
    prev = None
    for step in range(n_steps):
        if step % 20 == 0:
            be.thermal_cet(1e-6)
        if check_every_step:
            if step in Tsnap:
                assert np.array_equal(be.fields()[3], Tsnap[step]), f"T mismatch at step {step}"
            if step in Dsnap:
                assert np.array_equal(mask, Dsnap[step]), f"defect mask mismatch at step {step}"
        total, n_events, n_dep = be.sweep()
        assert n_events == int(z["n_events"][step]), (step, n_events, int(z["n_events"][step]))
        assert n_dep == int(z["n_dep"][step]), step
        ref_tot = float(z["seq_total"][step])
        assert abs(total - ref_tot) <= rate_rtol * abs(ref_tot), (step, total, ref_tot)
        if n_events == 0 or total < 1e-25 or not np.isfinite(total):
            break
        u_dep = np.random.random(n_dep)                    # kmc_event_rates.py:65, one per candidate
        ev = be.select(random.random() * total)            # kmc_simulation.py:265
        if ev.type == 0:
            ev.atom = dep_species(u_dep[ev.dep_rank], c)
        th = ph = 0.0
        if ev.type in (0, 2):
            th = np.random.uniform(0, np.pi)               # :283-284 / :308-309
            ph = np.random.uniform(0, 2 * np.pi)
        mk = bool(df > 0.0 and random.random() < df)       # :323
        if check_every_step:
            prev = tuple(a.copy() for a in be.fields()[:3])
        be.apply(ev, th, ph, mk)
        dt = max(-np.log(max(1e-12, random.random())) / total, 1e-12)   # :331
        total_time += dt
        if check_every_step:
            cur = be.fields()[:3]
            ch = np.flatnonzero((cur[0].ravel() != prev[0].ravel()) | (cur[1].ravel() != prev[1].ravel())
                                | (cur[2].ravel() != prev[2].ravel()))
            got = {int(fi): (int(cur[0].ravel()[fi]), float(cur[1].ravel()[fi]), float(cur[2].ravel()[fi])) for fi in ch}
            assert got == diffs.get(step, {}), (step, TYPE_NAMES[ev.type], got, diffs.get(step, {}))
        if step % 200 == 0:                                 # :335-338
            s_now = be.fields()[0].astype(np.int64)
            mask, _ = host_defects.introduce_defects(s_now, s_now, be.fields()[3], apply_to_state=False)
            be.set_defects(mask)
    st, th_, ph_, _ = be.fields()
    assert np.array_equal(st, z["final_state"])
    assert np.array_equal(th_, z["final_theta"]) and np.array_equal(ph_, z["final_phi"])
    assert total_time == float(z["total_time"])
    assert np.array_equal(np.array([random.random() for _ in range(4)]), z["py_next"])
    assert np.array_equal(np.random.random(4), z["np_next"])
    return be


class GpuBackend:
    """Backend protocol over cetkmc.Engine (single-step C-ABI entry points)."""

    def __init__(self, state, theta, phi, T, defects, impurity_c, n_slabs=1):
        import cetkmc
        self.e = cetkmc.Engine(int(state.shape[0]), impurity_c=impurity_c, n_slabs=n_slabs)
        self.e.upload(state, theta, phi, T, defects)

    def thermal_cet(self, dt):
        self.e.thermal_cet(dt, scrub_nan=True)

    def sweep(self):
        return self.e.rate_sweep()

    def select(self, r):
        return self.e.select(r)

    def apply(self, ev, theta_new, phi_new, make_defect):
        self.e.apply(ev, theta_new, phi_new, make_defect)

    def set_defects(self, mask):
        self.e.set_defects(mask)

    def fields(self):
        d = self.e.download()
        return d["state"], d["theta"], d["phi"], d["T"]


def random_lattice(L, seed, fill=0.3, t_lo=2600.0, t_hi=3690.0, hot_frac=0.05):
    """Synthetic lattice exercising all four event families (test-only generator)."""
    rs = np.random.RandomState(seed)
    state = np.zeros((L, L, L), dtype=np.int64)
    occ = rs.random_sample((L, L, L)) < fill
    species = rs.choice([1, 2, 3, 4], size=(L, L, L), p=[0.6, 0.15, 0.2, 0.05])
    state[occ] = species[occ]
    theta = np.where((state != 0) & (state != 4), rs.uniform(0, np.pi, (L, L, L)), 0.0)
    phi = np.where((state != 0) & (state != 4), rs.uniform(0, 2 * np.pi, (L, L, L)), 0.0)
    T = rs.uniform(t_lo, t_hi, (L, L, L))
    hot = rs.random_sample((L, L, L)) < hot_frac
    T[hot] = rs.uniform(3690.0, 4064.5, int(hot.sum()))
    defects = ((state == 3) & (rs.random_sample((L, L, L)) < 0.3)).astype(np.int64)
    return state, theta, phi, T, defects


# ---- batched stepping at 128 < L <= 256: deferred apply ("apply in sweep") ---------------------------
APPLY_IN_SWEEP_BATCHES = (7, 1, 13, 1, 20, 26, 2, 19, 3, 1)      # batches that start and end at many offsets modulo 20
FOUR_KIND_PARAMS = dict(I0=1e11)      # at the default I0 = 5e13 nucleation swamps diffusion and attachment; with 1e11 all four fire


def face_lattice(L, seed, n_atoms):
    """synthetic.planes plus n_atoms random atoms in the empty part, some on the lattice faces and in the top plane: events
    whose stale rows are clipped.  uint8 planes, as Engine.upload_planes takes them."""
    from cetkmc import synthetic
    st, th, ph, T, df = synthetic.planes(L, 0, L, seed=seed)
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, L, (n_atoms, 3))
    st[idx[:, 0], idx[:, 1], idx[:, 2]] = rs.randint(1, 5, n_atoms)
    for f in range(8):
        st[0, rs.randint(L), rs.randint(L)] = 1 + f % 3
        st[L - 1, rs.randint(L), rs.randint(L)] = 1 + f % 3
        st[rs.randint(L), 0, rs.randint(L)] = 1 + f % 3
        st[rs.randint(L), L - 1, rs.randint(L)] = 1 + f % 3
    return st, th, ph, T, df


def step_uniforms(seed, n, n_np):
    rs = np.random.RandomState(seed)
    return rs.random_sample(n), rs.random_sample(n), rs.random_sample(n_np)


def batch_calls(batches, seed0=100, step0=0):
    """(step0, n, u_pick, u_def, u_np) per batch, back to back from step0; rng_mode 1 streams (two orientation draws a step)."""
    calls, s = [], step0
    for k, n in enumerate(batches):
        calls.append((s, n) + step_uniforms(seed0 + k, n, 2 * n + 2))
        s += n
    return calls


def is_deferred(step0, n, x, thermal_mode=2):
    """Step x of a call of n steps from global step step0 launches its selection alone (its event is applied inside the next
    sweep launch) iff it is not the call's last step and the next step is no temperature-update step."""
    return x + 1 < n and not (thermal_mode and (step0 + x + 1) % 20 == 0)


def count_deferred(calls, thermal_mode=2):
    """What cetkmc_counters.deferred_steps holds after these calls on the deferring path: launches the host issued, so every
    step of every call counts, also behind an early stop."""
    return sum(is_deferred(c[0], c[1], x, thermal_mode) for c in calls for x in range(c[1]))


def oracle_lattice(oracle_mod, lat, impurity_c, tweak=None):
    st, th, ph, T, df = lat
    o = oracle_mod.Lattice(st.astype(np.int64), th, ph, T, df.astype(np.int64), impurity_c=impurity_c)
    for k, v in (tweak or {}).items():
        setattr(o.params, k, v)
    return o


def deferred_coverage(L, calls, logs, defect_fraction, thermal_mode=2):
    """What the deferred steps of a run exercised, from the ORACLE's per-call results ``logs`` (never the engine's): events
    of each kind, diffusions whose two sites lie in different rows / planes, events on the i and j faces (clipped patch),
    defect injections."""
    cov = dict(kinds=[0, 0, 0, 0], diff_rows=0, diff_planes=0, face_i=0, face_j=0, defects=0)
    for (step0, n, _, u_def, _), ro in zip(calls, logs):
        for x in range(ro["done"]):
            if not is_deferred(step0, n, x, thermal_mode):
                continue
            ev = ro["events"][x]
            t, pos, tgt = int(ev["type"]), ev["pos"], ev["target"]
            cov["kinds"][t] += 1
            if t == 1:
                cov["diff_rows"] += int(pos[0] != tgt[0] or pos[1] != tgt[1])
                cov["diff_planes"] += int(pos[0] != tgt[0])
            cov["face_i"] += int(pos[0] in (0, L - 1))
            cov["face_j"] += int(pos[1] in (0, L - 1))
            cov["defects"] += int(defect_fraction > 0.0 and u_def[x] < defect_fraction)
    return cov


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_fields_match_oracle(e, lat, rate_rtol, tag=""):
    """The lattice the engine (or ensemble replica) ``e`` holds against the oracle lattice ``lat``: all five fields (theta
    and phi by their bits, T with NaN == NaN, the defect mask) and the sweep of that lattice (counts, row counts, row sums,
    total)."""
    d = e.download(defects=True)
    assert np.array_equal(d["state"], lat.state), (tag, "state", np.argwhere(d["state"] != lat.state)[:4])
    assert np.array_equal(_bits(d["theta"]), _bits(lat.theta)), (tag, "theta")
    assert np.array_equal(_bits(d["phi"]), _bits(lat.phi)), (tag, "phi")
    assert np.array_equal(d["defects"], lat.defects), (tag, "defects")
    assert np.array_equal(d["T"], lat.T, equal_nan=True), (tag, "T")
    # sweep of the lattice the call left (state, rate table and interface sums as the batch's last apply kept them)
    sw = lat.sweep()
    total, n_events, n_dep = e.rate_sweep()
    rsum, rcnt = e.row_sums()
    assert (n_events, n_dep) == (sw["n_events"], sw["n_dep"]), (tag, n_events, n_dep, sw["n_events"], sw["n_dep"])
    assert np.array_equal(rcnt, sw["rowcnt"]), (tag, "rowcnt", np.argwhere(rcnt != sw["rowcnt"])[:4])
    fin = np.isfinite(sw["rowsum"])
    assert np.array_equal(np.isfinite(rsum), fin), (tag, "row sum finiteness")
    if fin.any():
        err = relerr(rsum[fin], sw["rowsum"][fin])
        assert err.max() <= rate_rtol, (tag, "rowsum", float(err.max()))
    if np.isfinite(sw["total"]):
        assert abs(total - sw["total"]) <= rate_rtol * abs(sw["total"]), (tag, total, sw["total"])


def assert_call_matches_oracle(e, lat, rg, ro, rate_rtol, tag=""):
    """One run_steps call of the engine ``e`` (result rg) against the same call of the oracle lattice ``lat`` (result ro):
    stop state, stream positions, event log, totals, the downloaded fields and the row sums of the lattice the call left."""
    for f in ("done", "status"):
        assert rg[f] == ro[f], (tag, f, rg[f], ro[f])
    # the log before the stream positions: a wrong step is reported as that step, not as what it did to the counts
    # (rng_mode 2 against the oracle's single-domain super-steps: that result has no stream position, deposition rank or
    # per-step event count; everything it has is compared)
    for f in ("type", "pos", "target", "atom") + (("dep_rank",) if "np_used" in ro else ()):
        if not np.array_equal(rg["events"][f], ro["events"][f]):
            x = [x for x in range(rg["done"]) if not np.array_equal(rg["events"][f][x], ro["events"][f][x])][0]
            raise AssertionError(f"{tag}: event field {f} differs first at step {x} of the call: "
                                 f"engine {rg['events'][x]} oracle {ro['events'][x]} (oracle's previous event: "
                                 f"{ro['events'][x - 1] if x else None})")
    for f in ("np_used", "q_used"):
        if f in ro:
            assert rg[f] == ro[f], (tag, f, rg[f], ro[f])
    assert rg["nucleation_count"] == lat.nuc_count, (tag, rg["nucleation_count"], lat.nuc_count)
    if "n_events" in ro:
        assert np.array_equal(rg["n_events"], ro["n_events"]), (tag, "n_events", np.flatnonzero(rg["n_events"] != ro["n_events"])[:4], rg["n_events"][:8], ro["n_events"][:8])
    assert len(rg["totals"]) == len(ro["totals"])
    if len(ro["totals"]):
        err = relerr(rg["totals"], ro["totals"])
        assert err.max() <= rate_rtol, (tag, "totals", int(err.argmax()), float(err.max()))
    assert_fields_match_oracle(e, lat, rate_rtol, tag)


def assert_ensemble_call_matches_oracle(ens, lats, res, oracle_results, rate_rtol, tag=""):
    """One cetkmc.Ensemble.run call (result ``res``) against the same call of every replica's own oracle lattice:
    ``oracle_results[r]`` is what lats[r].run_steps (rng_mode 0) or lats[r].run_supersteps(box == L) (rng_mode 2) returned,
    or None for a replica that was frozen when the call began (its oracle lattice was not stepped: status 1, no steps).
    Per replica: stop state, stream position (rng_mode 0), nucleation count, totals, the terminating total, the time
    increments (rng_mode 2), the selection margin, then the fields and the sweep of the lattice the call left."""
    assert len(lats) == len(oracle_results) == ens.R
    for r, (lat, ro) in enumerate(zip(lats, oracle_results)):
        t = f"{tag} replica {r}"
        done, status = (0, 1) if ro is None else (ro["done"], ro["status"])
        assert (int(res["done"][r]), int(res["status"][r])) == (done, status), (t, "done, status", res["done"][r], res["status"][r],
                                                                                done, status)
        if ro is not None and "np_used" in ro:
            assert int(res["np_used"][r]) == ro["np_used"], (t, "np_used", res["np_used"][r], ro["np_used"])
        assert int(res["nucleation_count"][r]) == lat.nuc_count, (t, "nucleation_count", res["nucleation_count"][r], lat.nuc_count)
        if done:
            err = relerr(res["totals"][r][:done], ro["totals"][:done])
            assert err.max() <= rate_rtol, (t, "totals", int(err.argmax()), float(err.max()))
        if ro is not None and status == 1:         # the total the termination branch saw: 0, below 1e-25 or not finite
            got, want = float(res["totals"][r][done]), float(ro["totals"][done])
            if np.isfinite(want):
                assert relerr([got], [want])[0] <= rate_rtol, (t, "terminating total", got, want)
            else:
                assert np.array_equal(got, want, equal_nan=True), (t, "terminating total", got, want)
        if ro is not None and "dt_event" in ro and done:
            err = relerr(res["dt"][r][:done], ro["dt_event"][:done])
            assert err.max() <= rate_rtol, (t, "dt", int(err.argmax()), float(err.max()))
        assert 0.0 < res["min_margin"][r] <= 1.0, (t, "min_margin", res["min_margin"][r])
        assert_fields_match_oracle(ens.replica(r), lat, rate_rtol, t)


def assert_supersteps_match_oracle(e, lat, rg, ro, rate_rtol, tag=""):
    """One run_supersteps call of the engine ``e`` (result rg, with want_events) against the same call of the oracle lattice
    ``lat`` (result ro): stop state, the per-box event log (idle boxes and null events included), executed counts, totals, the
    terminating total, time increments, nucleation count, then the fields and the sweep of the lattice the call left."""
    for f in ("done", "status"):
        assert rg[f] == ro[f], (tag, f, rg[f], ro[f])
    done = ro["done"]
    ge, oe = rg["events"], ro["events"]
    if ge.ndim == 1:                           # box == L: one Mode A event per super-step
        ge = ge.reshape(-1, 1)
    assert ge.shape == oe.shape, (tag, "event log shape", ge.shape, oe.shape)
    for f in ("type", "pos", "target", "atom"):
        if not np.array_equal(ge[f], oe[f]):
            bad = np.argwhere((ge[f] != oe[f]).reshape(ge.shape[0], ge.shape[1], -1).any(axis=2))[0]
            raise AssertionError(f"{tag}: event field {f} differs first at super-step {bad[0]} of the call, box {bad[1]}: "
                                 f"engine {ge[bad[0], bad[1]]} oracle {oe[bad[0], bad[1]]}")
    live = oe["type"] != -1                    # executed picks and null events (type -2) both carry their rate
    if live.any():
        err = relerr(ge["rate"][live], oe["rate"][live])
        assert err.max() <= rate_rtol, (tag, "event rates", float(err.max()))
    assert np.array_equal(rg["n_exec"], ro["n_exec"]), (tag, "n_exec", rg["n_exec"], ro["n_exec"])
    assert len(rg["totals"]) == len(ro["totals"]) and len(rg["dt_event"]) == len(ro["dt_event"]) == done, (tag, "log lengths")
    fin = np.isfinite(ro["totals"])
    assert np.array_equal(np.isfinite(rg["totals"]), fin), (tag, "totals finiteness")
    if fin.any():
        err = relerr(rg["totals"][fin], ro["totals"][fin])
        assert err.max() <= rate_rtol, (tag, "totals", int(err.argmax()), float(err.max()))
    if done:
        err = relerr(rg["dt_event"], ro["dt_event"])
        assert err.max() <= rate_rtol, (tag, "dt_event", int(err.argmax()), float(err.max()))
    assert rg["q_used"] == ro["q_used"], (tag, "q_used", rg["q_used"], ro["q_used"])
    assert rg["nucleation_count"] == lat.nuc_count, (tag, "nucleation_count", rg["nucleation_count"], lat.nuc_count)
    assert_fields_match_oracle(e, lat, rate_rtol, tag)


def assert_local_matches_ref(e, lat, rg, ro, rate_rtol, tag=""):
    """One run_supersteps_local call (result rg, with want_events) against tests/local_ref.run on the oracle lattice (ro), as
    tests/test_gpu_local_vs_ref.py compares: stop state, per-box event sequences, counts, totals, horizons, then the fields."""
    assert (rg["done"], rg["status"]) == (ro["done"], ro["status"]), (tag, rg["done"], rg["status"], ro["done"], ro["status"])
    done, ge, oe = ro["done"], rg["events"], ro["events"]
    assert ge.shape == oe.shape, (tag, "event log shape", ge.shape, oe.shape)
    for f in ("type", "pos", "target", "atom"):
        if not np.array_equal(ge[f], oe[f]):
            bad = np.argwhere((ge[f] != oe[f]).reshape(done, ge.shape[1], ge.shape[2], -1).any(axis=3))[0]
            raise AssertionError(f"{tag}: event field {f} differs first at super-step {bad[0]} of the call, box {bad[1]}, event {bad[2]}: "
                                 f"engine {ge[tuple(bad)]} comparator {oe[tuple(bad)]}")
    live = oe["type"] >= 0
    if live.any():
        assert relerr(ge["rate"][live], oe["rate"][live]).max() <= rate_rtol, (tag, "event rates")
        assert np.array_equal(ge["theta"][live], oe["theta"][live]) and np.array_equal(ge["phi"][live], oe["phi"][live]), (tag, "angles")
    assert np.array_equal(rg["n_exec"], ro["n_exec"]) and np.array_equal(rg["n_capped"], ro["n_capped"]), (tag, "n_exec, n_capped")
    assert len(rg["totals"]) == len(ro["totals"]), (tag, "log lengths")
    if len(ro["totals"]):
        assert relerr(rg["totals"], ro["totals"]).max() <= rate_rtol, (tag, "totals")
    if done:
        fin = np.isfinite(ro["horizon"])
        assert np.array_equal(np.isfinite(rg["horizon"]), fin) and np.array_equal(rg["horizon"][~fin], ro["horizon"][~fin]), (tag, "horizon")
        if fin.any():
            assert relerr(rg["horizon"][fin], ro["horizon"][fin]).max() <= rate_rtol, (tag, "horizon")
        assert relerr(rg["dt_event"], ro["dt_event"]).max() <= rate_rtol, (tag, "dt_event")
    assert rg["nucleation_count"] == lat.nuc_count, (tag, "nucleation_count", rg["nucleation_count"], lat.nuc_count)
    assert_fields_match_oracle(e, lat, rate_rtol, tag)
