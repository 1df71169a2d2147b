"""NumPy comparator of the layer profile (cetkmc_layer_profile) and the lattices its tests use.

``layer_ref`` restates the definition with whole-array comparisons of shifted label volumes -- no tiles, no ballots, no
partial records: nothing of the device kernel's structure.  Everything is integer counting, so the tests compare with ==.
"""
import numpy as np

FIELDS = ("n_occ", "n_start", "n_eq", "seg", "cut", "occ_state", "gb_state")


def grain_classes(bbox, ar_threshold):
    """eq[id] for id = 0..n (eq[0] = False): float(max(d)) / float(max(min(d), 1)) < ar_threshold over the bounding-box
    extents d -- the expression of metrics.compute_metrics_from_clusters."""
    bbox = np.asarray(bbox, dtype=np.int64).reshape(-1, 6)
    eq = np.zeros(len(bbox) + 1, bool)
    for q, b in enumerate(bbox.tolist()):
        d = [b[3 + a] - b[a] + 1 for a in range(3)]
        eq[q + 1] = float(max(d)) / float(max(min(d), 1)) < ar_threshold
    return eq


def layer_ref(labels, state, bbox, first, ar_threshold):
    """The per-plane counters of one lattice: dict of int64 arrays n_occ, n_start, n_eq (L,), seg, cut (L, 3), occ_state,
    gb_state (L, 4).  labels (L, L, L) int (0 = empty, ids 1..n), state (L, L, L), bbox (n, 6), first (n, 3)."""
    g = np.asarray(labels, dtype=np.int64)
    s = np.asarray(state, dtype=np.int64)
    L = g.shape[0]
    occ = g != 0
    eq = grain_classes(bbox, ar_threshold)

    def per_plane(mask):
        return mask.reshape(L, -1).sum(axis=1).astype(np.int64)

    start = np.zeros(g.shape, bool)
    for q, f in enumerate(np.asarray(first, dtype=np.int64).reshape(-1, 3).tolist()):
        assert g[tuple(f)] == q + 1
        start[tuple(f)] = True
    out = {"n_occ": per_plane(occ), "n_start": per_plane(start & occ), "n_eq": per_plane(occ & eq[g]),
           "seg": np.zeros((L, 3), np.int64), "cut": np.zeros((L, 3), np.int64),
           "occ_state": np.zeros((L, 4), np.int64), "gb_state": np.zeros((L, 4), np.int64)}
    differs = np.zeros(g.shape, bool)            # a face neighbour inside the lattice with another label
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, L - 1), slice(1, L)
        lo, hi = tuple(lo), tuple(hi)
        inside = np.zeros(g.shape, bool)         # the predecessor along axis a is inside the lattice
        inside[hi] = True
        pred = np.zeros_like(g)
        pred[hi] = g[lo]
        out["seg"][:, a] = per_plane(occ & (~inside | (pred != g)))
        out["cut"][:, a] = per_plane(occ & inside & (pred != 0) & (pred != g))
        differs[hi] |= g[hi] != g[lo]
        differs[lo] |= g[lo] != g[hi]
    for t in range(1, 5):
        out["occ_state"][:, t - 1] = per_plane(occ & (s == t))
        out["gb_state"][:, t - 1] = per_plane(occ & (s == t) & differs)
    return out


def same(got, want):
    """list of (field, plane) where two profiles differ (empty: equal in every counter)."""
    bad = []
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        bad += [(k, int(i)) for i in np.unique(np.argwhere(a != b)[:, 0])]
    return bad


# ---- lattices -----------------------------------------------------------------------------------------------------------
_DIAG = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], dtype=np.float64) / np.sqrt(3.0)


def diagonal_angles():
    """(theta, phi) of the eight cube diagonals: any two differ by acos(1/3) = 1.23 rad at least."""
    return np.arccos(_DIAG[:, 2]), np.arctan2(_DIAG[:, 1], _DIAG[:, 0])


def constructed(L, h=None, species=None):
    """Columnar below, equiaxed above: fully filled 2 x 2 columns of height h in the planes 0..h-1 (bounding box h x 2 x 2;
    h >= 6 gives AR >= 3), one empty plane h, 2^3 cubes from plane h + 1 up (AR <= 2; blocks cut by the lattice faces are
    smaller).  A block's orientation is the cube diagonal numbered by the parities of its block index, so every two blocks
    that touch -- diagonally too -- differ by 1.23 rad at least and same-coloured blocks are two blocks apart: no clustering
    threshold below 1.23 joins voxels of two blocks.  (Within a block the clustering's stencil joins the voxels of one
    i + j + k parity: the engine finds two grains per block, block_labels the idealised one.)  Returns state (int64),
    theta, phi, h.  ``species``: optional
    RandomState that draws the states 1..4 of the occupied voxels (default: all 1)."""
    if h is None:
        h = 6 if L >= 8 else max(L - 3, 1)
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    bi = np.where(i < h, 0, (i - (h + 1)) // 2 + 1)
    colour = (bi % 2) * 4 + ((j // 2) % 2) * 2 + (k // 2) % 2
    th, ph = diagonal_angles()
    state = np.where(i == h, 0, 1).astype(np.int64)
    if species is not None:
        state = np.where(state != 0, species.randint(1, 5, state.shape), 0).astype(np.int64)
    return state, np.ascontiguousarray(th[colour]), np.ascontiguousarray(ph[colour]), h


def random_blocks(L, seed, fill=0.7):
    """Random block lattice: boxes of random edge 1..4 per axis tile the lattice (cut positions drawn per axis), a block is
    filled with probability ``fill``, its orientation random; the states 1..4 drawn per voxel, all four present for
    L >= 2.  Returns state (int64), theta, phi."""
    rs = np.random.RandomState(seed)

    def ids(n):
        out, q = [], 0
        while len(out) < n:
            out += [q] * int(rs.randint(1, 5))
            q += 1
        return np.array(out[:n])
    a, b, c = ids(L), ids(L), ids(L)
    na, nb, nc = a.max() + 1, b.max() + 1, c.max() + 1
    filled = rs.random_sample((na, nb, nc)) < fill
    bt = np.arccos(rs.uniform(-1.0, 1.0, (na, nb, nc)))
    bp = rs.uniform(-np.pi, np.pi, (na, nb, nc))
    ix = np.ix_(a, b, c)
    occ = filled[ix]
    state = np.where(occ, rs.randint(1, 5, (L, L, L)), 0).astype(np.int64)
    if L >= 2 and occ.sum() >= 4:
        at = np.flatnonzero(occ.reshape(-1))
        state.reshape(-1)[rs.choice(at, 4, replace=False)] = np.arange(1, 5)
    return state, np.ascontiguousarray(bt[ix]), np.ascontiguousarray(bp[ix])


# the 14 neighbour offsets of the reference (kmc_event_rates.py): every one keeps the parity of i + j + k
STENCIL = ((1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1),
           (2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2))


def block_labels(L, h):
    """The grains of :func:`constructed` when every block is ONE grain (an idealised, face-connected labelling): labels
    numbered by first voxel in row-major order, first (n, 3), bbox (n, 6)."""
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    bi = np.where(i < h, 0, (i - (h + 1)) // 2 + 1)
    nb = (L + 1) // 2
    key = np.where(i == h, -1, (bi * nb + j // 2) * nb + k // 2)
    labels = np.zeros((L, L, L), np.int64)
    first, bbox, seen = [], [], {}
    for x in range(L ** 3):
        q = int(key.reshape(-1)[x])
        if q < 0:
            continue
        if q not in seen:
            seen[q] = len(seen) + 1
            first.append(np.unravel_index(x, (L, L, L)))
        labels.reshape(-1)[x] = seen[q]
    for q in range(1, len(seen) + 1):
        at = np.argwhere(labels == q)
        bbox.append(list(at.min(axis=0)) + list(at.max(axis=0)))
    return labels, np.array(first, np.int64).reshape(-1, 3), np.array(bbox, np.int64).reshape(-1, 6)


def host_clusters(state, theta, phi, threshold=0.5):
    """Connected components of the occupied voxels over the clustering's 14-stencil (STENCIL: the reference's neighbour
    list, which has no face neighbours) with misorientation below ``threshold`` -- a plain union-find for the host tests,
    numbered by first voxel in row-major order.  Returns labels, first (n, 3), size (n,), bbox (n, 6)."""
    L = state.shape[0]
    occ = np.asarray(state) != 0
    v = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=-1)
    parent = np.arange(L ** 3)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    idx = np.arange(L ** 3).reshape(L, L, L)
    for off in STENCIL:
        di, dj, dk = (int(x) for x in off)
        if (di, dj, dk) < (0, 0, 0):
            continue
        src = tuple(slice(max(0, -d), L - max(0, d)) for d in (di, dj, dk))
        dst = tuple(slice(max(0, d), L - max(0, -d)) for d in (di, dj, dk))
        dot = np.clip((v[src] * v[dst]).sum(axis=-1), -1.0, 1.0)
        join = occ[src] & occ[dst] & (np.arccos(dot) < threshold)
        for x, y in zip(idx[src][join].tolist(), idx[dst][join].tolist()):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    labels = np.zeros(L ** 3, np.int64)
    first, n = [], 0
    root_id = {}
    for x in np.flatnonzero(occ.reshape(-1)).tolist():
        r = find(x)
        if r not in root_id:
            n += 1
            root_id[r] = n
            first.append(np.unravel_index(x, (L, L, L)))
        labels[x] = root_id[r]
    labels = labels.reshape(L, L, L)
    size = np.zeros(n, np.int64)
    bbox = np.zeros((n, 6), np.int64)
    for q in range(1, n + 1):
        at = np.argwhere(labels == q)
        size[q - 1] = len(at)
        bbox[q - 1] = list(at.min(axis=0)) + list(at.max(axis=0))
    return labels, np.array(first, np.int64).reshape(n, 3), size, bbox
