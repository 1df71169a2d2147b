"""Comparator of the solidification-front diagnostics (cetkmc_front_stats, include/cetkmc.h).

Plain NumPy, the definition restated with its expression order.  The reference has no such function: this file IS the
definition's executable form, pinned on hand-computed cases by test_front_ref_host.py.

  front voxel  state != 0 and one of the six face neighbours INSIDE the lattice has state == 0
  gradient     along an axis at index x: (T[x+1] - T[x-1]) * (0.5 * inv_dx) inside, (T[1] - T[0]) * inv_dx at x == 0,
               (T[L-1] - T[L-2]) * inv_dx at x == L-1, 0.0 when L == 1;  G = sqrt(gi*gi + gj*gj + gk*gk), left to right
  skipped      a front voxel whose G or own T is not finite
  melt voxel   T >= T_melt, whatever the state (NaN is none, +inf is one)
"""
import math

import numpy as np

U = 2.0 ** -53          # unit roundoff of binary64


def gradient_component(T, axis, inv_dx):
    L = T.shape[axis]
    g = np.zeros_like(T)
    if L == 1:
        return g
    half_inv_dx = 0.5 * inv_dx
    Tm = np.moveaxis(T, axis, 0)
    gm = np.moveaxis(g, axis, 0)
    gm[1:-1] = (Tm[2:] - Tm[:-2]) * half_inv_dx
    gm[0] = (Tm[1] - Tm[0]) * inv_dx
    gm[-1] = (Tm[-1] - Tm[-2]) * inv_dx
    return g


def front_ref(state, T, T_melt, inv_dx):
    """Per-voxel fields of the definition: dict(front, skipped (disjoint boolean masks: front = front voxels NOT skipped),
    melt, G, gi, gj, gk)."""
    state = np.asarray(state)
    T = np.asarray(T, dtype=np.float64)
    occ, empty = state != 0, state == 0
    nb_empty = np.zeros(state.shape, bool)
    for axis in range(3):
        e = np.moveaxis(empty, axis, 0)
        n = np.moveaxis(nb_empty, axis, 0)
        n[:-1] |= e[1:]
        n[1:] |= e[:-1]
    cand = occ & nb_empty
    with np.errstate(invalid="ignore", over="ignore"):
        gi, gj, gk = (gradient_component(T, a, inv_dx) for a in range(3))
        G = np.sqrt(gi * gi + gj * gj + gk * gk)
        ok = np.isfinite(G) & np.isfinite(T)
        melt = T >= T_melt
    return dict(front=cand & ok, skipped=cand & ~ok, melt=melt, G=G, gi=gi, gj=gj, gk=gk)


def front_ref_stats(ref, T):
    """The fields of cetkmc_front_stats from front_ref's masks, the three sums with math.fsum (correctly rounded), plus
    abs_G / abs_gi / abs_T = fsum(|x|) for the summation bound."""
    T = np.asarray(T, dtype=np.float64)
    L = T.shape[0]
    f = ref["front"]
    idx = np.argwhere(f)
    G, gi, Tf = ref["G"][f], ref["gi"][f], T[f]
    m = np.argwhere(ref["melt"])
    bbox = np.array([L, L, L, -1, -1, -1], np.int32)
    if len(m):
        bbox = np.concatenate([m.min(axis=0), m.max(axis=0)]).astype(np.int32)
    n = int(f.sum())
    return dict(n_front=n, n_skipped=int(ref["skipped"].sum()),
                pos_sum=idx.sum(axis=0).astype(np.int64) if n else np.zeros(3, np.int64),
                G_sum=math.fsum(G), G_min=float(G.min()) if n else 0.0, G_max=float(G.max()) if n else 0.0,
                Gi_sum=math.fsum(gi), T_sum=math.fsum(Tf), n_melt=int(len(m)), melt_bbox=bbox,
                abs_G=math.fsum(np.abs(G)), abs_gi=math.fsum(np.abs(gi)), abs_T=math.fsum(np.abs(Tf)))


def sum_bound(n, abs_sum, per_term_ulp=False):
    """Worst case of ANY summation order of n terms against the correctly rounded sum: n * 2^-53 * sum|x|; with
    ``per_term_ulp`` each term may itself be off by 1 ulp (2^-52 relative: the square root of G)."""
    return n * U * abs_sum + (2.0 * U * abs_sum if per_term_ulp else 0.0)


def check_stats(got, want, what=""):
    """Assert one lattice's device result ``got`` (Engine.front_stats dict) against front_ref_stats ``want``: integer
    fields, G_min and G_max exactly (the device's f64 square root was measured to agree with NumPy's correctly rounded
    one in every case of the suite, DESIGN.md section 16: the 1-ulp allowance the definition grants is not used), the
    sums within sum_bound."""
    for k in ("n_front", "n_skipped", "n_melt"):
        assert int(got[k]) == int(want[k]), (what, k, int(got[k]), int(want[k]))
    assert np.array_equal(np.asarray(got["pos_sum"]), want["pos_sum"]), (what, "pos_sum", got["pos_sum"], want["pos_sum"])
    assert np.array_equal(np.asarray(got["melt_bbox"]), want["melt_bbox"]), (what, "melt_bbox", got["melt_bbox"], want["melt_bbox"])
    n = want["n_front"]
    for k in ("G_min", "G_max"):
        assert float(got[k]) == want[k], (what, k, float(got[k]), want[k])
    for k, a, ulp in (("G_sum", "abs_G", True), ("Gi_sum", "abs_gi", False), ("T_sum", "abs_T", False)):
        err, bound = abs(float(got[k]) - want[k]), sum_bound(n, want[a], ulp)
        assert err <= bound, (what, k, float(got[k]), want[k], err, bound)
