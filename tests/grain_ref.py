"""NumPy comparator of the per-grain table (cetkmc_grain_table) and the guards its tests call.

``grain_ref`` restates the definition with np.bincount over the labels of the occupied voxels and whole-array comparisons
of shifted views of the label volume padded with -1 by two cells -- no chunks, no waves, no slots: nothing of the device
kernel's structure.  The counters are integers, so the tests compare with ==; the two angles are copies and are compared as
int64 views.
"""
import numpy as np

import layer_ref as LR

INT_FIELDS = ("n", "sum", "sq", "n_state", "nb")
FIELDS = INT_FIELDS + ("first_theta", "first_phi")
STENCIL = LR.STENCIL
REC = 160                   # bytes of a record: 18 int64 counters and two doubles


def _by_label(idx, n, w=None):
    """sum of the integer weights w (default 1) per label index 0..n-1, exact: float64 partial sums stay below 2^53"""
    if w is None:
        return np.bincount(idx, minlength=n).astype(np.int64)
    assert float(np.abs(w).sum()) < 2.0 ** 53
    return np.rint(np.bincount(idx, weights=w.astype(np.float64), minlength=n)).astype(np.int64)


def grain_ref(labels, state, theta, phi):
    """The table of one lattice as Engine.grain_table returns it: dict of n (n,), sum (n, 3), sq (n, 6), n_state (n, 4),
    nb (n, 4) int64 and first_theta, first_phi (n,) float64.  labels (L, L, L) int, 0 = empty, ids 1..n."""
    g = np.asarray(labels, dtype=np.int64)
    s = np.asarray(state, dtype=np.int64)
    L = g.shape[0]
    n = int(g.max()) if g.size else 0
    occ = g > 0
    idx = g[occ] - 1
    co = [c[occ].astype(np.int64) for c in np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")]
    out = {"n": _by_label(idx, n),
           "sum": np.stack([_by_label(idx, n, c) for c in co], axis=1).reshape(n, 3),
           "sq": np.stack([_by_label(idx, n, co[a] * co[b]) for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))],
                          axis=1).reshape(n, 6),
           "n_state": np.stack([_by_label(idx, n, (s[occ] == t).astype(np.int64)) for t in (1, 2, 3, 4)], axis=1).reshape(n, 4)}
    pad = np.full((L + 4,) * 3, -1, np.int64)
    pad[2:L + 2, 2:L + 2, 2:L + 2] = g
    nb = np.zeros(4 * n, np.int64)
    own = g[occ]
    for d in STENCIL:
        u = pad[2 + d[0]:2 + d[0] + L, 2 + d[1]:2 + d[1] + L, 2 + d[2]:2 + d[2] + L][occ]
        cat = np.select([u == -1, u == 0, u == own], [3, 2, 0], default=1)       # outside, empty, same; otherwise other
        nb += _by_label(4 * idx + cat, 4 * n)
    out["nb"] = nb.reshape(n, 4)
    flat = g.reshape(-1)
    first = np.full(n, -1, np.int64)
    at = np.flatnonzero(flat)
    first[flat[at][::-1] - 1] = at[::-1]                 # the last write per label is its first voxel in row-major order
    assert (first >= 0).all()
    out["first_theta"] = np.asarray(theta, dtype=np.float64).reshape(-1)[first].copy()
    out["first_phi"] = np.asarray(phi, dtype=np.float64).reshape(-1)[first].copy()
    return out


def same(got, want):
    """names of the fields in which two tables differ (empty: equal in every bit)."""
    bad = []
    for k in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(k)
        elif k in INT_FIELDS:
            if a.dtype != np.int64 or not np.array_equal(a, b):
                bad.append(k)
        elif not np.array_equal(a.view(np.int64), b.view(np.int64)):
            bad.append(k)
    return bad


def as_bytes(t):
    return b"".join(np.ascontiguousarray(t[k]).tobytes() for k in FIELDS)


def check_identities(want, size=None, layer=None):
    """the identities of the definition; ``size``: the clustering's size table; ``layer``: the same lattice's layer profile"""
    assert np.array_equal(want["nb"].sum(axis=1), 14 * want["n"])
    assert int(want["nb"][:, 0].sum()) % 2 == 0
    assert (want["n"] >= 1).all() and (want["n_state"].sum(axis=1) <= want["n"]).all()
    if size is not None:
        assert np.array_equal(want["n"], np.asarray(size, dtype=np.int64))
    if layer is not None:
        assert int(want["n"].sum()) == int(layer["n_occ"].sum())
        assert np.array_equal(want["n_state"].sum(axis=0), layer["occ_state"].sum(axis=0))


# ---- what keeps a case from passing vacuously ----------------------------------------------------------------------------
# the kernel's edges (csrc/grain.hpp): a wave reads 64 consecutive voxels in row-major order, a pass of a block 256, a block
# GRAIN_VPB = 2048; a block's table in LDS has 128 slots
EDGES = (64, 256, 2048)
SLOTS = 128
# the shapes of the device comparison on imported labellings: layer_ref's, and the L whose L^3 lie on either side of a pass
# (6^3 < 256 < 7^3) and of a block (12^3 < 2048 < 13^3)
SHAPES = tuple(sorted(set(LR.SHAPES) | {6, 12, 13}))


def straddling_pairs(labels, edge):
    """(same, other): stencil pairs of labelled voxels whose linear indices lie in different chunks of ``edge`` voxels, with
    one label / with two."""
    g = np.asarray(labels, dtype=np.int64)
    L = g.shape[0]
    lin = np.arange(g.size, dtype=np.int64).reshape(g.shape)
    same_n = other_n = 0
    for d in STENCIL:
        if d < (0, 0, 0):
            continue
        sa = tuple(slice(max(0, -x), L - max(0, x)) for x in d)
        sb = tuple(slice(max(0, x), L - max(0, -x)) for x in d)
        if any(x.stop <= x.start for x in sa):
            continue
        a, b = g[sa], g[sb]
        across = (lin[sa] // edge != lin[sb] // edge) & (a > 0) & (b > 0)
        same_n += int((across & (a == b)).sum())
        other_n += int((across & (a != b)).sum())
    return same_n, other_n


def check_import(kind, L, labels, want):
    """an imported labelling of layer_ref.KINDS at L >= 4: same-label stencil pairs lie across the wave, pass and block
    edges of the lattice, and for ``scattered`` and ``blocks`` other-label pairs too; ``scattered`` fills all four contact
    categories.  ``one`` and ``scattered`` have them at every edge the lattice has.  The slabs and boxes of the other kinds
    are product partitions: where the lattice has ONE edge of a size, that edge may fall between two boxes or into an empty
    slab (stripes0 at L = 13, blocks at L = 8), so they are asked for the edge sizes that occur more than once."""
    if L < 4:
        return
    assert int(want["nb"][:, 0].sum()) > 0, (kind, L)
    for edge in EDGES:
        if L ** 3 > (edge if kind in ("one", "scattered") else 2 * edge):
            s, o = straddling_pairs(labels, edge)
            assert s > 0, (kind, L, edge)
            if kind in ("scattered", "blocks") and L >= 7:
                assert o > 0, (kind, L, edge)
    if kind == "one":
        assert len(want["n"]) == 1 and int(want["n"][0]) == L ** 3 and not want["nb"][:, 1:3].any()
    if kind == "scattered" and L >= 7:
        assert (want["nb"].sum(axis=0) > 0).all() and (want["n"] > 1).any()


def check_clustered(want, largest=None, full=False):
    """a table of the device clustering's: all four contact categories (``full``: a lattice without an empty voxel has the
    other three), grains of more than one voxel and, where the family promises one, a largest grain of at least ``largest``
    of the occupied voxels."""
    tot = want["nb"].sum(axis=0)
    assert (tot[[0, 1, 3]] > 0).all() and (tot[2] == 0 if full else tot[2] > 0)
    assert (want["n"] > 1).any()
    if largest is not None:
        assert float(want["n"].max()) / float(want["n"].sum()) >= largest


def singletons(L, fill=0.7, seed=5):
    """every occupied voxel its own grain (ids in row-major order).  Returns labels (int32), state."""
    rs = np.random.RandomState(seed)
    occ = rs.random_sample((L, L, L)) < fill
    lab = np.zeros(L ** 3, np.int32)
    at = np.flatnonzero(occ.reshape(-1))
    lab[at] = np.arange(1, len(at) + 1)
    return lab.reshape(L, L, L), LR._species(rs, occ)


def angles(L, seed):
    """theta, phi on every voxel, a few of them not finite."""
    rs = np.random.RandomState(seed)
    th, ph = rs.uniform(0.0, np.pi, (L, L, L)), rs.uniform(0.0, 2.0 * np.pi, (L, L, L))
    bad = (np.nan, np.inf, -np.inf)
    for q in range(min(6, L ** 3)):
        (th if q % 2 else ph).reshape(-1)[(q * 7919) % L ** 3] = bad[q % 3]
    return th, ph
