"""Beam tables: the definition in executable form.  NumPy on oracle.Lattice arrays; never touches the
engine.  Built on tests/implicit_ref.py (scrub, clip, Stepper) and tests/boundary_ref.py (coefficients, solves, addends).

A beam table is dict(u0, amp (n_u), gj (n_u, L), gk (n_u, L), fi (D)), every value finite and >= 0.  The source of update
ordinal u is row x = u - u0; voxel (i, j, k) at depth d = L - 1 - i receives
  qv    = (amp[x] * fi[d]) * (gj[x][j] * gk[x][k])  if d < D else 0.0        three multiplies, one IEEE operation per NumPy call
  qterm = qv / rho_cp  where qv != 0.0, else 0.0
and everything else is boundary_ref.step: b = scrub(T) + dt * (qterm + latent_coef * dF), the solves along axes 2, 1, 0 with the
boundary's diagonals and addends (None: adiabatic, section 26's arithmetic), the clip, prev_state := state.  u is the update
ordinal in every respect: the boundary's face temperatures are those of u too (a stepping call: u = g // 20).
"""
import numpy as np

import boundary_ref
import implicit_ref


def check(t, L):
    """what the library refuses"""
    n_u, D = t["amp"].size, t["fi"].size
    if n_u < 1 or not 1 <= D <= L or t["gj"].shape != (n_u, L) or t["gk"].shape != (n_u, L):
        raise ValueError("beam table: n_u >= 1, 1 <= depth <= L, gj and gk (n_u, L)")
    for n in ("amp", "gj", "gk", "fi"):
        if not (np.isfinite(t[n]).all() and (t[n] >= 0.0).all()):
            raise ValueError(f"beam table: {n} holds a negative or non-finite value")


def row_of(t, u):
    x = int(u) - t["u0"]
    if not 0 <= x < t["amp"].size:
        raise ValueError(f"update ordinal {u} outside the table's rows [{t['u0']}, {t['u0'] + t['amp'].size})")
    return x


def source(t, L, x):
    """qv of every voxel, (L, L, L)"""
    D = t["fi"].size
    qv = np.zeros((L, L, L))
    plane = t["gj"][x][:, None] * t["gk"][x][None, :]             # gj[j] * gk[k]
    for d in range(D):
        a = np.float64(t["amp"][x]) * np.float64(t["fi"][d])       # amp * fi[d]
        qv[L - 1 - d] = a * plane
    return qv


def product_plane(t, x):
    """the plane q[j][k] = (amp[x] * 1.0) * (gj[x][j] * gk[x][k]) that section 26's update equals a D = 1, fi = [1.0] beam on"""
    return (np.float64(t["amp"][x]) * np.float64(1.0)) * (t["gj"][x][:, None] * t["gk"][x][None, :])


def footprint_rows(t, L, x):
    """(L, L) bool per (plane, row): the rows a kernel must give their terms in full -- amp * fi[d] != 0 and gj[j] != 0"""
    need = np.zeros((L, L), bool)
    for d in range(t["fi"].size):
        if np.float64(t["amp"][x]) * np.float64(t["fi"][d]) != 0.0:
            need[L - 1 - d] = t["gj"][x] != 0.0
    return need


def qterm_of(lat, t, x):
    with np.errstate(all="ignore"):
        qv = source(t, lat.L, x)
        return np.where(qv != 0.0, qv / np.float64(lat.params.rho_cp), 0.0)


def rhs(lat, dt, t, x, latent, scrub):
    """the right-hand side of one implicit step: implicit_ref.rhs with the plane's term replaced by the table's"""
    P = lat.params
    tc = implicit_ref.scrub_field(lat.T, P) if scrub else lat.T.copy()
    L = lat.L
    qterm = qterm_of(lat, t, x)
    with np.errstate(all="ignore"):
        dF = np.zeros((L, L, L))
        if latent:
            dF[(lat.prev_state == 0) & (lat.state != 0)] = np.float64(1.0) / np.float64(max(dt, 1e-12))
        return tc + np.float64(dt) * (qterm + np.float64(P.latent_coef) * dF)


def step(lat, dt, t, x, bc=None, u=0, latent=False, scrub=False):
    """one implicit step of length dt from row x, the boundary's face temperatures those of update ordinal u; returns b"""
    P = lat.params
    b = rhs(lat, dt, t, x, latent, scrub)
    r = (np.float64(P.alpha) * np.float64(dt)) * np.float64(P.inv_dx2)
    beta = np.zeros(6) if bc is None else np.asarray(bc["beta"], np.float64)
    c = boundary_ref.addends(bc, r, u)
    v = b
    for axis in (2, 1, 0):
        if bc is None:
            inv, p = implicit_ref.coeffs(lat.L, r)
            v = implicit_ref.solve(v, axis, r, inv, p)
        else:
            inv, p = boundary_ref.coeffs(lat.L, r, beta[2 * axis], beta[2 * axis + 1])
            v = boundary_ref.solve(v, axis, r, inv, p, c[2 * axis], c[2 * axis + 1])
    v = np.where(v < P.T_clip_lo, P.T_clip_lo, v)
    lat.T = np.ascontiguousarray(np.where(v > P.T_clip_hi, P.T_clip_hi, v))
    if latent:
        lat.prev_state = lat.state.copy()
    return b


def update(lat, n, dt, t, u, use_latent=True, scrub=True, stats=None, bc=None):
    """one temperature update of ordinal u in n implicit steps of dt / n from the same row; stats as implicit_ref.update"""
    x = row_of(t, u)
    dt_s = dt / n if n > 1 else dt
    lo, hi = lat.params.T_clip_lo, lat.params.T_clip_hi
    if stats is not None:
        stats["updates"] += 1
        stats["substeps"] += n
        stats["nan_before"] += int(np.isnan(lat.T).sum())
        stats["inf_before"] += int(np.isinf(lat.T).sum())
        stats["source"] += int(np.any(source(t, lat.L, x) != 0.0))
        if use_latent:
            stats["latent"] += int(((lat.prev_state == 0) & (lat.state != 0)).sum())
    for s in range(n):
        first = s == 0
        step(lat, dt_s, t, x, bc, u, latent=bool(use_latent and first), scrub=bool(scrub and first))
        if stats is not None:
            stats["on_clip_lo"] = max(stats["on_clip_lo"], int((lat.T == lo).sum()))
            stats["on_clip_hi"] = max(stats["on_clip_hi"], int((lat.T == hi).sum()))


class _NoPlanes:
    """what a stepping call with a beam hands the loop for q_planes: nothing to index"""

    def __getitem__(self, q):
        return None


class Stepper(boundary_ref.Stepper):
    """boundary_ref.Stepper whose thermal_mode 2 updates take their source from the table row of u = g // 20, however the run is
    cut into calls; thermal_mode 1 updates are boundary_ref's.  ``beam_updates`` counts the updates made from the table."""

    def __init__(self, lat, t, n=1, threshold=None, bc=None):
        super().__init__(lat, n, threshold, bc)
        self.table, self.beam_updates = t, 0

    def _update(self, lat, n, dt, thermal_mode, q, **kw):
        if thermal_mode != 2:
            return super()._update(lat, n, dt, thermal_mode, q, **kw)
        g = self._gs.pop(0)
        update(lat, n, dt, self.table, g // 20, bc=self.bc, **kw)
        self.bc_updates += boundary_ref.active(self.bc)
        self.beam_updates += 1

    def run_steps(self, step0, n, *args, **kw):
        if kw.get("thermal_mode", 1) == 2:
            assert kw.get("q_planes") is None, "a beam: no planes"
            kw["q_planes"] = _NoPlanes()
        return super().run_steps(step0, n, *args, **kw)
