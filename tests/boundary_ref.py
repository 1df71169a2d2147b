"""Thermal boundary conditions of the implicit scheme: the definition in executable form.  NumPy on
oracle.Lattice arrays; never touches the engine.  Built on tests/implicit_ref.py (right-hand side, scrub, clip, Stepper).

Six faces in the order FACES (face 2 * axis + hi; i_lo the substrate side, i_hi plane L - 1).  Face f carries beta >= 0, T_ext
and ramp; the voxel on the face sees a ghost node of value x + beta * (T_f - x), T_f = T_ext + ramp * u for update ordinal u
(u = g // 20 in a stepping call, 0 for a direct update).  One implicit step is implicit_ref.step with, per axis (lo, hi):
  diagonal      row 0: 1 + r (1 + beta_lo), row L - 1: 1 + r (1 + beta_hi), L = 1: 1 + r (beta_lo + beta_hi)
  right side    c_f = (r * beta_f) * T_f;  y[0] = (b[0] + c_lo) inv[0],  y[L - 1] = ((b[L - 1] + c_hi) + r y[L - 2]) inv[L - 1],
                L = 1: ((b + c_lo) + c_hi) inv[0]; an addend only where beta_f != 0
A boundary is None (adiabatic) or dict(beta=, T_ext=, ramp=) of six floats each.
"""
import numpy as np

import implicit_ref

FACES = ("i_lo", "i_hi", "j_lo", "j_hi", "k_lo", "k_hi")


def boundary(beta=None, T_ext=None, ramp=None, **faces):
    """dict(beta, T_ext, ramp); ``faces``: name=(beta, T_ext) or (beta, T_ext, ramp) for single faces"""
    b = dict(beta=np.zeros(6) if beta is None else np.array(beta, np.float64).reshape(6),
             T_ext=np.zeros(6) if T_ext is None else np.array(T_ext, np.float64).reshape(6),
             ramp=np.zeros(6) if ramp is None else np.array(ramp, np.float64).reshape(6))
    for name, v in faces.items():
        f = FACES.index(name)
        b["beta"][f], b["T_ext"][f] = v[0], v[1]
        b["ramp"][f] = v[2] if len(v) > 2 else 0.0
    return b


def active(bc):
    return bc is not None and bool(np.any(np.asarray(bc["beta"]) != 0.0))


def face_T(bc, u):
    """T_f of update ordinal u: one multiply, one add; not clipped"""
    with np.errstate(all="ignore"):
        return np.asarray(bc["T_ext"], np.float64) + np.asarray(bc["ramp"], np.float64) * np.float64(u)


def coeffs(L, r, beta_lo=0.0, beta_hi=0.0):
    """(inv, p) of the Thomas algorithm for one axis with faces (lo, hi)"""
    L, r, bl, bh = int(L), np.float64(r), np.float64(beta_lo), np.float64(beta_hi)
    if L < 1 or not np.isfinite(r) or r < 0:
        raise ValueError("coeffs: L >= 1 and a finite r >= 0")
    if not (np.isfinite(bl) and np.isfinite(bh)) or bl < 0 or bh < 0:
        raise ValueError("coeffs: finite beta >= 0")
    one, two = np.float64(1.0), np.float64(2.0)
    inv, p = np.zeros(L), np.zeros(L)
    inv[0] = one / ((one + r * (bl + bh)) if L == 1 else (one + r * (one + bl)))
    p[0] = r * inv[0]
    for m in range(1, L):
        diag = (one + two * r) if m < L - 1 else (one + r * (one + bh))
        inv[m] = one / (diag - r * p[m - 1])
        p[m] = r * inv[m]
    return inv, p


def solve(b, axis, r, inv, p, c_lo=None, c_hi=None):
    """the solve of one axis along every line; c_lo / c_hi: the end addends, None on an adiabatic face"""
    r = np.float64(r)
    y = np.moveaxis(np.array(b, np.float64), axis, 0).copy()
    L = y.shape[0]
    with np.errstate(all="ignore"):
        if c_lo is not None:
            y[0] = y[0] + np.float64(c_lo)
        if c_hi is not None:
            y[L - 1] = y[L - 1] + np.float64(c_hi)          # L = 1: (b + c_lo) + c_hi
        y[0] = y[0] * inv[0]
        for m in range(1, L):
            y[m] = (y[m] + r * y[m - 1]) * inv[m]
        for m in range(L - 2, -1, -1):
            y[m] = y[m] + p[m] * y[m + 1]
    return np.ascontiguousarray(np.moveaxis(y, 0, axis))


def addends(bc, r, u):
    """[c_f or None] for the six faces"""
    if bc is None:
        return [None] * 6
    Tf = face_T(bc, u)
    with np.errstate(all="ignore"):
        return [None if bc["beta"][f] == 0.0 else (np.float64(r) * np.float64(bc["beta"][f])) * Tf[f] for f in range(6)]


def step(lat, dt, bc=None, u=0, thermal_mode=1, q=None, latent=False, scrub=False):
    """one implicit step of length dt with the boundary; returns (b, per-axis solutions) for the tests that look inside"""
    P = lat.params
    b = implicit_ref.rhs(lat, dt, thermal_mode, q, latent, scrub)
    r = (np.float64(P.alpha) * np.float64(dt)) * np.float64(P.inv_dx2)
    beta = np.zeros(6) if bc is None else np.asarray(bc["beta"], np.float64)
    c = addends(bc, r, u)
    x, stages = b, []
    for axis in (2, 1, 0):
        inv, p = coeffs(lat.L, r, beta[2 * axis], beta[2 * axis + 1])
        x = solve(x, axis, r, inv, p, c[2 * axis], c[2 * axis + 1])
        stages.append(x)
    v = np.where(x < P.T_clip_lo, P.T_clip_lo, x)
    lat.T = np.ascontiguousarray(np.where(v > P.T_clip_hi, P.T_clip_hi, v))
    if thermal_mode == 2 and latent:
        lat.prev_state = lat.state.copy()
    return b, stages


def update(lat, n, dt, thermal_mode=1, q=None, use_latent=True, scrub=True, stats=None, bc=None, u=0):
    """one temperature update in n implicit steps of dt / n with the same T_f; stats as implicit_ref.update"""
    dt_s = dt / n if n > 1 else dt
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
        step(lat, dt_s, bc, u, thermal_mode, q, latent=bool(use_latent and first and thermal_mode == 2), scrub=bool(scrub and first))
        if stats is not None:
            stats["on_clip_lo"] = max(stats["on_clip_lo"], int((lat.T == lo).sum()))
            stats["on_clip_hi"] = max(stats["on_clip_hi"], int((lat.T == hi).sum()))


class Stepper(implicit_ref.Stepper):
    """implicit_ref.Stepper with the boundary: the update of global step g uses T_f of u = g // 20, however the run is cut into
    calls.  ``bc_updates`` counts the updates made with a non-adiabatic boundary."""

    def __init__(self, lat, n=1, threshold=None, bc=None):
        super().__init__(lat, n, threshold, update_fn=self._update)
        self.bc, self.bc_updates, self._gs = bc, 0, []

    def _update(self, lat, n, dt, thermal_mode, q, **kw):
        g = self._gs.pop(0)
        update(lat, n, dt, thermal_mode, q, bc=self.bc, u=g // 20, **kw)
        self.bc_updates += active(self.bc)

    def run_steps(self, step0, n, *args, **kw):
        first = step0 + (-step0) % 20       # the update steps of the call, less the one a stopped call has already applied
        self._gs = [g for g in range(first, step0 + n, 20) if not (g == step0 and g == self.applied_g)]
        return super().run_steps(step0, n, *args, **kw)
