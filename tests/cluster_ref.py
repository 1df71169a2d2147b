"""Independent comparator of the grain clustering (cetkmc_cluster, Ensemble.analyze, utils.get_clusters) and the inputs its
tests use.  NumPy + SciPy; nothing of utils.py or csrc/cluster.hpp is used or restated.

``cluster_ref`` states the definition as a graph problem: the nodes are the occupied voxels, an edge joins two occupied
voxels that differ by one of the 14 stencil offsets and whose orientations are closer than the threshold, the grains are the
connected components (scipy.sparse.csgraph), numbered 1..n by their first voxel in row-major order.  The seven forward offsets
are applied to whole arrays by slicing; there is no traversal, no stack and no union-find here.

The edge predicate is decided in cosine space in long double: join <=> dot > cos(threshold) for 0 < threshold <= pi, nothing
joins for threshold <= 0, every pair with a finite dot product joins for threshold > pi; a NaN dot product never joins.  The
code under test works in double (unit vectors from sin / cos, three products, acos), which errs by about 1e-15 in the dot
product, so a pair whose dot product lies within ``GUARD`` = 1e-12 of cos(threshold) could be decided either way; such pairs
are counted (``ambiguous``) and every test asserts that its input has none.  An input that has one is replaced by another
input; the guard stays.
"""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

GUARD = 1e-12
LD = np.longdouble
# the forward half of the 14-offset stencil (the other seven are these negated)
FORWARD = ((1, 1, 0), (1, -1, 0), (0, 1, 1), (0, 1, -1), (2, 0, 0), (0, 2, 0), (0, 0, 2))


def unit_vectors(theta, phi):
    """(N, 3) long double unit vectors (sin t cos p, sin t sin p, cos t) of the flattened angles."""
    t, p = np.asarray(theta, np.float64).ravel().astype(LD), np.asarray(phi, np.float64).ravel().astype(LD)
    with np.errstate(invalid="ignore"):
        st = np.sin(t)
        return np.stack([st * np.cos(p), st * np.sin(p), np.cos(t)], axis=1)


def occupied_pairs(occ):
    """(a, b): linear indices of every pair of occupied voxels with b = a + a forward offset (each stencil pair once)."""
    shape = occ.shape
    lin = np.arange(occ.size, dtype=np.int64).reshape(shape)
    aa, bb = [], []
    for off in FORWARD:
        sa = tuple(slice(max(0, -d), n - max(0, d)) for d, n in zip(off, shape))
        sb = tuple(slice(max(0, d), n - max(0, -d)) for d, n in zip(off, shape))
        if any(s.stop <= s.start for s in sa):
            continue
        both = occ[sa] & occ[sb]
        aa.append(lin[sa][both])
        bb.append(lin[sb][both])
    if not aa:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(aa), np.concatenate(bb)


def decide(dot, threshold):
    """(join, n_ambiguous) of long double dot products at a threshold (module docstring)."""
    thr = float(threshold)
    with np.errstate(invalid="ignore"):
        if thr <= 0.0:
            return np.zeros(dot.shape, bool), 0
        if thr > np.pi:
            return np.isfinite(dot), 0
        c = np.cos(LD(thr))
        return dot > c, int(np.count_nonzero(np.abs(dot - c) < LD(GUARD)))


def cluster_ref(state, theta, phi, threshold):
    """The clustering of one lattice.  dict: labels (shape of state) int32, size (n,) int64, first (n, 3) int32, bbox (n, 6)
    int32 (min3, max3), ambiguous (int), and the pair list the helpers below read: a, b (linear indices), join (bool)."""
    state = np.asarray(state)
    shape = state.shape
    occ = state != 0
    a, b = occupied_pairs(occ)
    v = unit_vectors(theta, phi)
    with np.errstate(invalid="ignore"):
        dot = (v[a] * v[b]).sum(axis=1) if len(a) else np.zeros(0, LD)
    join, n_amb = decide(dot, threshold)
    n = state.size
    g = coo_matrix((np.ones(int(join.sum()), np.int8), (a[join], b[join])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    where = np.flatnonzero(occ.ravel())                 # occupied voxels in row-major order
    labels = np.zeros(n, np.int32)
    if len(where) == 0:
        return dict(labels=labels.reshape(shape), size=np.zeros(0, np.int64), first=np.zeros((0, 3), np.int32),
                    bbox=np.zeros((0, 6), np.int32), ambiguous=n_amb, a=a, b=b, join=join)
    _, first_at, inverse = np.unique(comp[where], return_index=True, return_inverse=True)
    rank = np.empty(len(first_at), np.int64)
    rank[np.argsort(first_at, kind="stable")] = np.arange(len(first_at))       # components in the order of their first voxel
    lab = rank[inverse] + 1
    labels[where] = lab
    k = len(first_at)
    coords = np.stack(np.unravel_index(where, shape), axis=1).astype(np.int32)
    order = np.argsort(lab, kind="stable")
    size = np.bincount(lab, minlength=k + 1)[1:].astype(np.int64)
    starts = np.concatenate(([0], np.cumsum(size)[:-1]))
    sc = coords[order]
    bbox = np.concatenate([np.minimum.reduceat(sc, starts, axis=0), np.maximum.reduceat(sc, starts, axis=0)], axis=1)
    return dict(labels=labels.reshape(shape), size=size, first=sc[starts], bbox=bbox.astype(np.int32), ambiguous=n_amb,
                a=a, b=b, join=join)


# ---- what keeps a case from passing vacuously ----------------------------------------------------------------------------
def chained_pairs(res):
    """stencil pairs of occupied voxels in ONE grain whose own predicate is false: they are joined only through others."""
    lab = res["labels"].ravel()
    return int(np.count_nonzero((lab[res["a"]] == lab[res["b"]]) & ~res["join"]))


def largest_share(res):
    """the largest grain's share of the occupied voxels (0.0 for an empty lattice)."""
    return float(res["size"].max()) / float(res["size"].sum()) if len(res["size"]) else 0.0


def join_degree(res):
    """per voxel (flattened), the number of its stencil neighbours it is joined to."""
    n = res["labels"].size
    j = res["join"]
    return np.bincount(res["a"][j], minlength=n) + np.bincount(res["b"][j], minlength=n)


def nonfinite_next_to_finite(state, theta, phi):
    """occupied voxels with a non-finite angle that have an occupied stencil neighbour with finite angles."""
    state = np.asarray(state)
    occ = state != 0
    a, b = occupied_pairs(occ)
    fin = (np.isfinite(theta) & np.isfinite(phi)).ravel()
    return int(len(np.unique(np.concatenate([a[~fin[a] & fin[b]], b[~fin[b] & fin[a]]]))))


def same(got, want):
    """names of the fields in which an engine's clustering differs from the comparator's (empty: equal everywhere)."""
    bad = []
    if not (got["labels"].dtype == np.int32 and np.array_equal(got["labels"], want["labels"])):
        bad.append("labels")
    for k in ("size", "first", "bbox"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape or not np.array_equal(g, w):
            bad.append(k)
    return bad


def from_host(clusters, visited):
    """utils.get_clusters' return value in the comparator's layout (labels, size, first, bbox)."""
    n = len(clusters)
    bbox = np.zeros((n, 6), np.int32)
    for q, c in enumerate(clusters):
        xyz = np.asarray(c, np.int32).reshape(-1, 3)
        bbox[q, :3], bbox[q, 3:] = xyz.min(axis=0), xyz.max(axis=0)
    return dict(labels=np.asarray(visited, np.int32), size=np.array([len(c) for c in clusters], np.int64),
                first=np.array([c[0] for c in clusters], np.int32).reshape(-1, 3), bbox=bbox)


# ---- the conditions of the input families (asserted without a GPU in test_cluster_ref_host.py, and again in the GPU tests) ----
def check_general(ref, L, threshold):
    assert ref["ambiguous"] == 0
    assert chained_pairs(ref) > 0
    if threshold == 1.2 and L >= 33:
        assert largest_share(ref) >= 0.10


def check_serpentine(ref, occ, n_paths):
    L = occ.shape[0]
    assert ref["ambiguous"] == 0
    assert len(ref["size"]) == n_paths and int(ref["size"].sum()) == int(occ.sum())
    assert join_degree(ref).max() <= 2
    for q in range(n_paths):                                    # every occupied plane, from the first to the last
        planes = np.unique(np.argwhere(ref["labels"] == q + 1)[:, 0])
        assert np.array_equal(planes, np.arange(0, 4 * ((L - 1) // 4) + 1, 2)), q
        assert ref["bbox"][q, 0] == 0 and ref["bbox"][q, 3] == 4 * ((L - 1) // 4)


def check_textured(ref):
    assert ref["ambiguous"] == 0
    assert chained_pairs(ref) > 0
    assert largest_share(ref) >= 0.10


def check_ensemble(name, r, state, ref):
    """replica r of ensemble case ``name`` (ENSEMBLES below): L30_R6 has an empty replica (2) and one of singletons (3);
    every other replica has chained pairs; every replica of L64_R3 percolates at its threshold."""
    assert ref["ambiguous"] == 0, (name, r)
    n_occ = int((np.asarray(state) != 0).sum())
    assert int(ref["size"].sum()) == n_occ
    if name == "L30_R6" and r == 2:
        assert n_occ == 0 and len(ref["size"]) == 0
    elif name == "L30_R6" and r == 3:
        assert len(ref["size"]) == n_occ > 0
    else:
        assert chained_pairs(ref) > 0, (name, r)
    if name == "L64_R3":
        assert largest_share(ref) >= 0.10, (name, r)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def species(rng, occ):
    """int64 state: 0 where not occ, species 1..4 elsewhere."""
    state = np.zeros(occ.shape, np.int64)
    state[occ] = rng.choice([1, 2, 3, 4], size=int(occ.sum()), p=[0.6, 0.15, 0.2, 0.05])
    return state


def continuous(L, fill, seed):
    """(state, theta, phi): a fraction ``fill`` occupied, theta ~ U(0, pi), phi ~ U(0, 2 pi) on EVERY voxel (the empty ones
    carry orientations too: they must not matter), from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    state = species(rng, rng.random((L, L, L)) < fill)
    return state, rng.uniform(0.0, np.pi, (L, L, L)), rng.uniform(0.0, 2.0 * np.pi, (L, L, L))


def textured(L=33, fill=0.7, seed=330, spread=0.3):
    """continuous orientations within +-spread of one direction: misorientations between 0 and about 0.8, so the product's
    fixed threshold 0.5 joins most neighbours (one grain percolates) but not all (chained pairs)."""
    rng = np.random.default_rng(seed)
    state = species(rng, rng.random((L, L, L)) < fill)
    return state, 1.0 + rng.uniform(-spread, spread, (L, L, L)), 2.0 + rng.uniform(-spread, spread, (L, L, L))


# (L, fill, threshold, seed) of the general single-lattice cases; the 1.2 cases at L >= 33 percolate
GENERAL = ((7, 0.9, 0.5, 7), (16, 0.7, 1.2, 16), (33, 0.6, 0.9, 33), (64, 0.6, 1.2, 64), (130, 0.6, 1.2, 130), (130, 0.6, 0.5, 130))

EDGE_L = 20
EDGE_THRESHOLDS = (-1.0, 0.0, 0.1, float(np.pi), 4.0)


def edge_lattice(seed=20):
    """L = 20, fill 0.8: half of the voxels take one of 4 palette orientations (dot products of exactly equal vectors), half
    continuous ones; 40 occupied voxels get a NaN / +inf / -inf theta or phi."""
    L = EDGE_L
    rng = np.random.default_rng(seed)
    state = species(rng, rng.random((L, L, L)) < 0.8)
    theta, phi = rng.uniform(0.0, np.pi, (L, L, L)), rng.uniform(0.0, 2.0 * np.pi, (L, L, L))
    pal_t, pal_p = rng.uniform(0.0, np.pi, 4), rng.uniform(0.0, 2.0 * np.pi, 4)
    pick, use = rng.integers(0, 4, (L, L, L)), rng.random((L, L, L)) < 0.5
    theta, phi = np.where(use, pal_t[pick], theta), np.where(use, pal_p[pick], phi)
    at = rng.choice(np.flatnonzero(state.ravel()), size=40, replace=False)
    bad = np.array([np.nan, np.inf, -np.inf])
    for q, x in enumerate(at):
        (theta if q % 2 else phi).ravel()[x] = bad[q % 3]
    return state, theta, phi


PLANT_L = 26
PLANT_DELTAS = (1e-9, 1e-10)


def planted_pairs(threshold, seed=26):
    """(state, theta, phi, pairs): 28 pairs of voxels, each alone in empty space (anchors 6 apart, so no voxel of one pair
    is a stencil neighbour of another pair's): one per forward offset, per sign and per delta in PLANT_DELTAS, with equal phi
    and theta differing by threshold - delta (sign -1: joins) or threshold + delta (sign +1: does not).  ``pairs``: list of
    (voxel a, voxel b, sign)."""
    L = PLANT_L
    rng = np.random.default_rng(seed)
    state = np.zeros((L, L, L), np.int64)
    theta, phi = np.zeros((L, L, L)), np.zeros((L, L, L))
    pairs, q = [], 0
    for off in FORWARD:
        for sign in (-1, 1):
            for delta in PLANT_DELTAS:
                a = (2 + 6 * (q % 4), 2 + 6 * ((q // 4) % 4), 2 + 6 * (q // 16))
                b = tuple(x + d for x, d in zip(a, off))
                t0, p0 = rng.uniform(0.3, 2.0), rng.uniform(0.0, 2.0 * np.pi)
                state[a], state[b] = 1 + q % 4, 1 + (q + 1) % 4
                theta[a], theta[b] = t0, t0 + (float(threshold) + sign * delta)
                phi[a] = phi[b] = p0
                pairs.append((a, b, sign))
                q += 1
    return state, theta, phi, pairs


CONST_THRESHOLD = 4.0        # with one constant orientation every occupied stencil pair joins: no floating point in the predicate


def constant(occ, t=0.7, p=2.1):
    """(state 1 where occ, theta = t, phi = p everywhere)"""
    occ = np.asarray(occ, bool)
    return occ.astype(np.int64), np.full(occ.shape, t), np.full(occ.shape, p)


def mod4(L):
    """voxels with all three coordinates = 0 mod 4: no two are stencil neighbours."""
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    return (i % 4 == 0) & (j % 4 == 0) & (k % 4 == 0)


def serpentine(L, shift=0):
    """One thin path: rows along k (every second voxel: the (0, 0, 2) offset) at j = 0, 4, 8, .., joined at alternate ends by
    one connector voxel at j + 2; planes i = 0, 4, 8, .. traversed in alternating j order and joined by one connector voxel at
    i + 2.  The first voxel is one end; every voxel is joined to at most two others.  ``shift``: the k columns used are
    shift, shift + 2, ..: serpentine(L, 0) | serpentine(L, 1) are two disjoint interleaved paths."""
    occ = np.zeros((L, L, L), bool)
    ks = list(range(shift, L, 2))
    js = list(range(0, L, 4))
    planes = list(range(0, L, 4))
    at_end = False              # the k end of the path: False = ks[0], True = ks[-1]
    for pi, i in enumerate(planes):
        rows = js if pi % 2 == 0 else js[::-1]
        for ri, j in enumerate(rows):
            occ[i, j, ks] = True
            at_end = not at_end
            if ri + 1 < len(rows):
                occ[i, (j + rows[ri + 1]) // 2, ks[-1] if at_end else ks[0]] = True
        if pi + 1 < len(planes):
            occ[i + 2, rows[-1], ks[-1] if at_end else ks[0]] = True
    return occ


# ---- ensembles: (L, thresholds) -> list of replicas (state, theta, phi, T) ------------------------------------------------
ENSEMBLES = {"L30_R6": (30, (0.5, 1.2)), "L64_R3": (64, (1.2,)), "L17_R2": (17, (0.5,))}


def ensemble_lattices(name):
    """The replicas of one ensemble case, all different.  L30_R6: continuous 0.7 / full continuous / EMPTY / mod-4 singletons
    with one orientation / continuous 0.5 / continuous 0.9 -- the empty one in the middle, so that the concatenated stats
    table has a zero-length entry between others.  T carries NaN and +-inf at some species-3 voxels."""
    L = ENSEMBLES[name][0]
    if name == "L30_R6":
        reps = [continuous(L, 0.7, 301), continuous(L, 1.0, 302), continuous(L, 0.0, 303), None, continuous(L, 0.5, 305),
                continuous(L, 0.9, 306)]
        st, th, ph = constant(mod4(L))
        reps[3] = (st * 3, th, ph)
    elif name == "L64_R3":
        reps = [continuous(L, 0.6, 641), continuous(L, 0.6, 642), continuous(L, 0.75, 643)]
    else:
        reps = [continuous(L, 0.8, 171), continuous(L, 0.6, 172)]
    out = []
    for r, (st, th, ph) in enumerate(reps):
        rng = np.random.default_rng(9000 + r)
        T = rng.uniform(2600.0, 3690.0, st.shape)
        c3 = np.flatnonzero(st.ravel() == 3)
        T.ravel()[c3[::7]] = np.nan
        T.ravel()[c3[3::7]] = np.inf
        T.ravel()[c3[5::7]] = -np.inf
        out.append((st, th, ph, T))
    return out


# ---- site queries ---------------------------------------------------------------------------------------------------------
SITE_L = 70


def site_lattices():
    """Two (state, theta, phi, T, defects) at L = 70: "mixed" holds species 1, 2 and 3 but no 4 (a gather of nothing), "one"
    is entirely species 2 (a gather of all L^3 voxels).  T holds NaN, +inf and -inf in every species."""
    L = SITE_L
    rng = np.random.default_rng(70)
    mixed = np.zeros((L, L, L), np.int64)
    occ = rng.random((L, L, L)) < 0.5
    mixed[occ] = rng.choice([1, 2, 3], size=int(occ.sum()), p=[0.6, 0.15, 0.25])
    out = {}
    for name, state in (("mixed", mixed), ("one", np.full((L, L, L), 2, np.int64))):
        T = rng.uniform(2600.0, 3690.0, (L, L, L))
        T.ravel()[::11] = np.nan
        T.ravel()[3::13] = np.inf
        T.ravel()[5::17] = -np.inf
        out[name] = (state, rng.uniform(0.0, np.pi, (L, L, L)), rng.uniform(0.0, 2.0 * np.pi, (L, L, L)), T, np.zeros_like(state))
    return out
