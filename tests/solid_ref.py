"""NumPy comparator of the solidification map (cetkmc_solid_*, include/cetkmc.h).

The reference has no such function: this file IS the definition's executable form, pinned on hand-computed cases by
test_solid_ref_host.py.  Whole-array operations only -- no pairs, waves, slots: nothing of the device kernels' structure.

  map      per voxel stamp (int64, -1 = no record) and five doubles T_s, gi, gj, gk, cool; a snapshot of state and of T.
  begin    stamp = -1, the doubles +0.0, snapshot = the current state and T (occupied voxels are substrate: no record).
  update   with s0 the snapshot state and s1 the current state of a voxel:
             s0 == 0 and s1 != 0   stamp = the call's stamp, T_s = T, (gi, gj, gk) = front_ref.gradient_component of T
                                   (central differences * (0.5 * inv_dx) inside, one-sided * inv_dx at the faces, 0.0 for
                                   L == 1), cool = (T - T_snap) / dt; non-finite results are stored as they come; n_new += 1
             s0 != 0 and s1 == 0   stamp = -1, the doubles +0.0; n_cleared += 1 (a substrate voxel counts, too)
             anything else         untouched (a change of species included)
           then snapshot = state, T_snap = T; n_recorded = voxels with stamp >= 0.
  profile  x0 = G = sqrt(gi*gi + gj*gj + gk*gk) (left to right), x1 = gi, x2 = cool, x3 = T_s; a recorded voxel is GOOD when
           the four x are finite and every |x_c * qscale[c]| < 2^38.  Per plane i and per label id > 0, over the good
           voxels: n_rec, stamp_sum, stamp_min, stamp_max, q[c] = sum of rint(x_c * qscale[c]) (round to nearest even),
           n_cooling (cool < 0); every other recorded voxel: n_bad.  Empty: stamp_min = INT64_MAX, stamp_max = -1.
"""
import numpy as np

from front_ref import gradient_component

LIM = 2.0 ** 38
NONE_MIN, NONE_MAX = np.iinfo(np.int64).max, -1
FIELDS = ("n_rec", "n_bad", "n_cooling", "stamp_sum", "stamp_min", "stamp_max", "q")
REC = 80                    # bytes of a record: ten int64
MAP_FIELDS = ("T_s", "g", "cool")


class SolidRef:
    def __init__(self, state, T):
        self.begin(state, T)

    @classmethod
    def from_map(cls, m):
        """a comparator holding the map ``m`` (Engine.solid_read) -- for profiles, which are defined given the map"""
        L = m["stamp"].shape[0]
        ref = cls(np.zeros((L, L, L), np.int64), np.zeros((L, L, L)))
        ref.stamp, ref.T_s, ref.g, ref.cool = (np.array(m[k]) for k in ("stamp", "T_s", "g", "cool"))
        return ref

    def begin(self, state, T):
        state = np.asarray(state)
        L = state.shape[0]
        self.L = L
        self.stamp = np.full((L, L, L), -1, np.int64)
        self.T_s = np.zeros((L, L, L))
        self.g = np.zeros((L, L, L, 3))
        self.cool = np.zeros((L, L, L))
        self.snap = state.copy()
        self.T_snap = np.array(T, dtype=np.float64)

    def update(self, state, T, stamp, inv_dx, dt):
        """One update; returns dict(n_new, n_cleared, n_recorded)."""
        assert stamp >= 0 and np.isfinite(dt) and dt > 0 and np.isfinite(inv_dx)
        state = np.asarray(state)
        T = np.asarray(T, dtype=np.float64)
        new = (self.snap == 0) & (state != 0)
        clr = (self.snap != 0) & (state == 0)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            g = np.stack([gradient_component(T, a, inv_dx) for a in range(3)], axis=-1)
            cool = (T - self.T_snap) / dt
        self.stamp[new] = stamp
        self.T_s[new] = T[new]
        self.g[new] = g[new]
        self.cool[new] = cool[new]
        self.stamp[clr] = -1
        self.T_s[clr] = 0.0
        self.g[clr] = 0.0
        self.cool[clr] = 0.0
        self.snap = state.copy()
        self.T_snap = T.copy()
        return dict(n_new=int(new.sum()), n_cleared=int(clr.sum()), n_recorded=int((self.stamp >= 0).sum()))

    def map(self):
        return dict(stamp=self.stamp, T_s=self.T_s, g=self.g, cool=self.cool)

    # -- profile -----------------------------------------------------------------------------------------------------------
    def quantities(self):
        """the four x of every voxel, (L, L, L, 4)"""
        gi, gj, gk = self.g[..., 0], self.g[..., 1], self.g[..., 2]
        with np.errstate(invalid="ignore", over="ignore"):
            G = np.sqrt(gi * gi + gj * gj + gk * gk)
        return np.stack([G, gi, self.cool, self.T_s], axis=-1)

    def good(self, scales, x=None):
        x = self.quantities() if x is None else x
        with np.errstate(invalid="ignore", over="ignore"):
            y = x * np.asarray(scales, dtype=np.float64)
            return (self.stamp >= 0) & np.isfinite(x).all(axis=-1) & (np.abs(y) < LIM).all(axis=-1)

    def profile(self, scales, labels=None):
        """dict(layers=records with leading dimension L, grains=records per label id 1..max (None without labels))."""
        x = self.quantities()
        rec = self.stamp >= 0
        ok = self.good(scales, x)
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.where(ok[..., None], np.rint(np.where(ok[..., None], x * np.asarray(scales, dtype=np.float64), 0.0)), 0.0).astype(np.int64)
        plane = np.broadcast_to(np.arange(self.L).reshape(-1, 1, 1), rec.shape)
        out = dict(layers=self._reduce(plane, self.L, rec, ok, q), grains=None)
        if labels is not None:
            lab = np.asarray(labels, dtype=np.int64)
            n = int(lab.max()) if lab.size else 0
            out["grains"] = self._reduce(lab - 1, n, rec & (lab > 0), ok & (lab > 0), q)
        return out

    def _reduce(self, key, n, rec, ok, q):
        r = dict(n_rec=np.zeros(n, np.int64), n_bad=np.zeros(n, np.int64), n_cooling=np.zeros(n, np.int64),
                 stamp_sum=np.zeros(n, np.int64), stamp_min=np.full(n, NONE_MIN, np.int64), stamp_max=np.full(n, NONE_MAX, np.int64),
                 q=np.zeros((n, 4), np.int64))
        k = key[ok]
        np.add.at(r["n_rec"], k, 1)
        np.add.at(r["n_bad"], key[rec & ~ok], 1)
        np.add.at(r["n_cooling"], key[ok & (self.cool < 0)], 1)
        np.add.at(r["stamp_sum"], k, self.stamp[ok])
        np.minimum.at(r["stamp_min"], k, self.stamp[ok])
        np.maximum.at(r["stamp_max"], k, self.stamp[ok])
        np.add.at(r["q"], k, q[ok])
        return r

    def ties(self, scales, eps=1e-6):
        """Voxels whose quantisation the definition leaves open: a recorded voxel where some x_c * qscale[c] lies within eps
        of a half-integer or of the 2^38 limit, or where that holds for G one ulp up or down (the definition grants the root
        1 ulp, as DESIGN.md section 16 does).  The tests assert this is 0 for their inputs before they compare."""
        x = self.quantities()
        rec = self.stamp >= 0
        s = np.asarray(scales, dtype=np.float64)
        bad = np.zeros(rec.shape, bool)
        with np.errstate(invalid="ignore", over="ignore"):
            variants = [x]
            for side in (np.inf, -np.inf):
                v = x.copy()
                v[..., 0] = np.nextafter(x[..., 0], side)
                variants.append(v)
            for v in variants:
                y = v * s
                fin = np.isfinite(y)
                frac = np.abs(y - np.floor(y) - 0.5)
                bad |= (fin & (frac < eps)).any(axis=-1)
                bad |= (fin & (np.abs(np.abs(y) - LIM) < 1.0)).any(axis=-1)
        return int((bad & rec).sum())


def check_identities(ref, prof, scales=None, labels=None):
    """n_recorded == sum over planes of (n_rec + n_bad); with labels: sum over planes of n_rec == sum over grains of n_rec +
    the good recorded voxels with label 0."""
    lay = prof["layers"]
    assert int(lay["n_rec"].sum()) + int(lay["n_bad"].sum()) == int((ref.stamp >= 0).sum())
    if labels is not None:
        unlabelled = int((ref.good(scales) & (np.asarray(labels) == 0)).sum())
        assert int(lay["n_rec"].sum()) == int(prof["grains"]["n_rec"].sum()) + unlabelled


def same_records(got, want):
    """names of the fields in which two record sets differ (empty: equal in every bit)."""
    bad = []
    for k in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != np.int64 or b.dtype != np.int64 or not np.array_equal(a, b):
            bad.append(k)
    return bad


def same_map(got, want):
    """names of the map arrays in which the device's map ``got`` (Engine.solid_read) differs from the comparator's: stamps
    ==; finite doubles as int64 views; non-finite ones by class (NaN against NaN, infinities with their sign)."""
    bad = []
    if not np.array_equal(np.asarray(got["stamp"]), want["stamp"]) or np.asarray(got["stamp"]).dtype != np.int64:
        bad.append("stamp")
    for k in MAP_FIELDS:
        a, b = np.ascontiguousarray(got[k], dtype=np.float64), np.ascontiguousarray(want[k], dtype=np.float64)
        if a.shape != b.shape:
            bad.append(k)
            continue
        fin = np.isfinite(b)
        ok = np.array_equal(np.isfinite(a), fin) and np.array_equal(a.view(np.int64)[fin], b.view(np.int64)[fin])
        ok = ok and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b)) \
            and np.array_equal(np.isneginf(a), np.isneginf(b))
        if not ok:
            bad.append(k)
    return bad


# ---- inputs of the device tests --------------------------------------------------------------------------------------------
# powers of two: with temperatures on a grid of 1/8 K, inv_dx = 1 and dt a power of two, gi, cool and T_s times their scale are
# integers (no tie can occur); only G, a square root, lands between the integers, and ties() looks at it
GRID_SCALES = (1024.0, 16.0, 2.0 ** -16, 8.0)


def grid_T(L, seed, levels=8, base=3000.0):
    """temperatures base + n / 8, n in [0, levels): differences are exact"""
    return base + np.random.RandomState(seed).randint(0, levels, (L, L, L)) / 8.0


def special_voxels(L):
    """the corners, the edge mid points and the face centres of the lattice (deduplicated; everything for L <= 2)"""
    c = sorted({0, L // 2, L - 1})
    pts = {(i, j, k) for i in c for j in c for k in c if (i in (0, L - 1)) or (j in (0, L - 1)) or (k in (0, L - 1))}
    return sorted(pts)


def sequence(L, seed, n_updates=3, fill=0.35, flip=0.15, T=grid_T):
    """states and temperatures of a begin and n_updates updates: [(state, T)] * (1 + n_updates).  Between two consecutive
    states a share ``flip`` of the empty voxels fills, the same share of the occupied ones empties and another one changes
    species; the special voxels (faces, edges, corners) alternate empty / occupied from an empty start, so they solidify,
    clear and solidify again."""
    rs = np.random.RandomState(seed)
    st = np.where(rs.random_sample((L, L, L)) < fill, rs.randint(1, 5, (L, L, L)), 0).astype(np.int64)
    sp = tuple(np.array(special_voxels(L)).T)
    out = []
    for u in range(n_updates + 1):
        if u:
            r = rs.random_sample((L, L, L))
            fresh = rs.randint(1, 5, (L, L, L))
            st = np.where((st == 0) & (r < flip), fresh, np.where((st != 0) & (r < flip), 0,
                          np.where((st != 0) & (r > 1.0 - flip), 1 + (st % 4), st))).astype(np.int64)
        st[sp] = (1 + u % 3) if u % 2 else 0
        out.append((st.copy(), T(L, seed * 131 + u)))
    return out
