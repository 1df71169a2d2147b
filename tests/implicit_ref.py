"""Implicit temperature updates: the definition in executable form.  NumPy on oracle.Lattice arrays;
never touches the engine.

One implicit step of length dt on a field T:
  1. b = scrub(T) + dt * (qterm + latent_coef * dF)   (laser mode; diffusion-only mode: b = scrub(T))
  2. (I - r D) x = b along axis 2, then axis 1, then axis 0, r = (alpha * dt) * inv_dx2, by the Thomas algorithm with
     ``coeffs(L, r)`` -- every line strictly in order, one IEEE operation per NumPy call, so a device that performs the same
     multiplies and adds without contraction produces the same bits
  3. the clip, once
  4. latent term on: prev_state := state
``update(lat, n, dt, ...)`` is one update in n such steps of dt / n, the first with the scrub and the latent term.  ``Stepper``
is the stepping loop composed from it, built like tests/substep_ref.Stepper.
"""
import numpy as np

from remelt_ref import remelt, updates_in
from substep_ref import new_stats


def coeffs(L, r):
    """(inv, p) of the Thomas algorithm for (I - r D) on a line of L voxels with replicated edges; L = 1: the identity"""
    L, r = int(L), np.float64(r)
    if L < 1 or not np.isfinite(r) or r < 0:
        raise ValueError("coeffs: L >= 1 and a finite r >= 0")
    one = np.float64(1.0)
    inv, p = np.zeros(L), np.zeros(L)
    inv[0] = one if L == 1 else one / (one + r)
    p[0] = r * inv[0]
    for m in range(1, L):
        beta = ((one + np.float64(2.0) * r) if m < L - 1 else (one + r)) - r * p[m - 1]
        inv[m] = one / beta
        p[m] = r * inv[m]
    return inv, p


def solve(b, axis, r, inv, p):
    """(I - r D) x = b along every line of ``axis``"""
    r = np.float64(r)
    y = np.moveaxis(np.array(b, np.float64), axis, 0).copy()
    L = y.shape[0]
    with np.errstate(all="ignore"):
        y[0] = y[0] * inv[0]
        for m in range(1, L):
            y[m] = (y[m] + r * y[m - 1]) * inv[m]
        for m in range(L - 2, -1, -1):
            y[m] = y[m] + p[m] * y[m + 1]
    return np.ascontiguousarray(np.moveaxis(y, 0, axis))


def scrub_field(T, params):
    """the scrub of this scheme: NaN -> T_nan, +inf -> T_clip_hi, -inf -> T_clip_lo; finite values untouched"""
    T = np.where(np.isnan(T), params.T_nan, T)
    T = np.where(T == np.inf, params.T_clip_hi, T)
    return np.where(T == -np.inf, params.T_clip_lo, T)


def rhs(lat, dt, thermal_mode, q, latent, scrub):
    """the right-hand side of one implicit step, thermal_voxel()'s source and latent-heat terms in its order"""
    P = lat.params
    tc = scrub_field(lat.T, P) if scrub else lat.T.copy()
    if thermal_mode != 2:
        return tc
    L = lat.L
    q = np.asarray(q, np.float64).reshape(L, L)
    qterm = np.zeros((L, L, L))
    with np.errstate(all="ignore"):
        qterm[L - 1] = np.where(q != 0.0, q / np.float64(P.rho_cp), 0.0)
        dF = np.zeros((L, L, L))
        if latent:
            dF[(lat.prev_state == 0) & (lat.state != 0)] = np.float64(1.0) / np.float64(max(dt, 1e-12))
        return tc + np.float64(dt) * (qterm + np.float64(P.latent_coef) * dF)


def step(lat, dt, thermal_mode=1, q=None, latent=False, scrub=False):
    """one implicit step of length dt; returns b (for the tests that look at the right-hand side)"""
    P = lat.params
    b = rhs(lat, dt, thermal_mode, q, latent, scrub)
    r = (np.float64(P.alpha) * np.float64(dt)) * np.float64(P.inv_dx2)
    inv, p = coeffs(lat.L, r)
    x = b
    for axis in (2, 1, 0):
        x = solve(x, axis, r, inv, p)
    v = np.where(x < P.T_clip_lo, P.T_clip_lo, x)
    lat.T = np.ascontiguousarray(np.where(v > P.T_clip_hi, P.T_clip_hi, v))
    if thermal_mode == 2 and latent:
        lat.prev_state = lat.state.copy()
    return b


def update(lat, n, dt, thermal_mode=1, q=None, use_latent=True, scrub=True, stats=None):
    """One temperature update of ``lat`` (oracle.Lattice) in n implicit steps of dt / n.  stats (substep_ref.new_stats()) is
    added to as tests/substep_ref.update does."""
    dt_s = dt / n if n > 1 else dt                  # one IEEE division, as the host does
    lo, hi = lat.params.T_clip_lo, lat.params.T_clip_hi
    if stats is not None:
        stats["updates"] += 1
        stats["substeps"] += n
        stats["nan_before"] += int(np.isnan(lat.T).sum())
        stats["inf_before"] += int(np.isinf(lat.T).sum())
        if thermal_mode == 2:
            stats["source"] += int(np.any(np.asarray(q) != 0.0))
            if use_latent:
                stats["latent"] += int(((lat.prev_state == 0) & (lat.state != 0)).sum())
    for s in range(n):
        first = s == 0
        step(lat, dt_s, thermal_mode, q, latent=bool(use_latent and first and thermal_mode == 2), scrub=bool(scrub and first))
        if stats is not None:
            stats["on_clip_lo"] = max(stats["on_clip_lo"], int((lat.T == lo).sum()))
            stats["on_clip_hi"] = max(stats["on_clip_hi"], int((lat.T == hi).sum()))


class Stepper:
    """The stepping loop of one lattice under the implicit scheme with thermal_substeps = n (and, with a threshold, remelting
    on): the update, then the melt, in front of every step with g % 20 == 0, then oracle steps with thermal_mode 0.
    ``update_fn`` replaces the update (tests/test_implicit_ref_host.py substitutes the explicit one to pin the plumbing)."""

    def __init__(self, lat, n=1, threshold=None, update_fn=None):
        self.lat, self.n, self.threshold = lat, int(n), threshold
        self.update_fn = update if update_fn is None else update_fn
        self.applied_g = -1         # a call that stopped with status 2 ON an update step has applied that step's whole update
        self.stats = new_stats()
        self.info = dict(passes=0, n_melted=0, n_melted_last=0)

    def melt(self, g):
        k = remelt(self.lat, self.threshold)
        self.info["passes"] += 1
        self.info["n_melted"] += k
        self.info["n_melted_last"] = k
        return k

    def run_steps(self, step0, n, defect_fraction, u_pick, u_defect, u_np, rng_mode=0, seed=0, thermal_mode=1, thermal_dt=1e-6,
                  q_planes=None, use_latent=True):
        lat = self.lat
        skip_g, self.applied_g = self.applied_g, -1
        u_np = np.zeros(0) if u_np is None else np.asarray(u_np, np.float64)
        s, np_pos, q_idx, status = 0, 0, 0, 0
        totals, events, nev, dts = [], [], [], []
        while s < n and status == 0:
            g = step0 + s
            if thermal_mode and g % 20 == 0:
                if s == 0 and g == skip_g:
                    q_idx += thermal_mode == 2          # its plane was consumed by the stopped call; no update
                else:
                    self.update_fn(lat, self.n, thermal_dt, thermal_mode, None if thermal_mode == 1 else q_planes[q_idx],
                                   use_latent=use_latent, scrub=True, stats=self.stats)
                    q_idx += thermal_mode == 2
                    if self.threshold is not None:
                        self.melt(g)
            nxt = min(n, s + 20 - g % 20) if thermal_mode else n
            m = nxt - s
            if rng_mode == 2:
                r = lat.run_supersteps(g, m, lat.L, defect_fraction, seed, thermal_mode=0, want_events=True)
                events.append(r["events"].reshape(-1))
                dts.append(r["dt_event"])
            else:
                r = lat.run_steps(g, m, defect_fraction, u_pick[s:nxt], None if u_defect is None else u_defect[s:nxt],
                                  u_np[np_pos:], rng_mode=rng_mode, seed=seed, thermal_mode=0)
                events.append(r["events"])
                nev.append(r["n_events"])
                np_pos += r["np_used"]
            totals.append(r["totals"])
            s += r["done"]
            status = r["status"]
        if status == 2 and thermal_mode and s < n and (step0 + s) % 20 == 0:
            self.applied_g = step0 + s
        out = dict(done=s, status=status,
                   q_used=0 if thermal_mode != 2 else updates_in(step0, n if status == 0 else min(s + 1, n)),
                   totals=np.concatenate(totals) if totals else np.zeros(0),
                   events=np.concatenate(events) if events else np.zeros(0, dtype=[("type", "<i4")]))
        if rng_mode == 2:
            out["dt_event"] = np.concatenate(dts) if dts else np.zeros(0)
        else:
            out["np_used"] = np_pos
            out["n_events"] = np.concatenate(nev) if nev else np.zeros(0, np.int64)
        return out
