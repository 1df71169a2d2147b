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


def _boxes(rs, L, fill):
    """the box partition of :func:`random_blocks`: per axis the box index of every coordinate (boxes of random edge 1..4),
    and which boxes are filled."""
    def ids(n):
        out, q = [], 0
        while len(out) < n:
            out += [q] * int(rs.randint(1, 5))
            q += 1
        return np.array(out[:n])
    a, b, c = ids(L), ids(L), ids(L)
    filled = rs.random_sample((a.max() + 1, b.max() + 1, c.max() + 1)) < fill
    return a, b, c, filled


def random_blocks(L, seed, fill=0.7):
    """Random block lattice: boxes of random edge 1..4 per axis tile the lattice (cut positions drawn per axis), a block is
    filled with probability ``fill``, its orientation random; the states 1..4 drawn per voxel, all four present for
    L >= 2.  Returns state (int64), theta, phi."""
    rs = np.random.RandomState(seed)
    a, b, c, filled = _boxes(rs, L, fill)
    na, nb, nc = filled.shape
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


def _block_key(L, h):
    """the block of every voxel of :func:`constructed` (any order of numbering); -1 in the empty plane h."""
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    bi = np.where(i < h, 0, (i - (h + 1)) // 2 + 1)
    nb = (L + 1) // 2
    return np.where(i == h, -1, (bi * nb + j // 2) * nb + k // 2)


def block_labels(L, h):
    """The grains of :func:`constructed` when every block is ONE grain (an idealised, face-connected labelling): labels
    numbered by first voxel in row-major order, first (n, 3), bbox (n, 6)."""
    key = _block_key(L, h)
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


# ---- labellings of the caller's (cetkmc_cluster_import) --------------------------------------------------------------------
def from_raw(raw):
    """Any non-negative integer volume (0 = empty; equal values = one grain, connected or not) as an importable labelling:
    labels renumbered 1..n by first occurrence in row-major order, first (n, 3), size (n,), bbox (n, 6).  Whole-array
    operations only."""
    raw = np.asarray(raw)
    assert raw.ndim == 3 and (raw >= 0).all()
    flat = raw.reshape(-1)
    vals, at, inv = np.unique(flat, return_index=True, return_inverse=True)
    keep = vals != 0
    n = int(keep.sum())
    lut = np.zeros(len(vals), np.int64)
    lut[np.flatnonzero(keep)[np.argsort(at[keep])]] = np.arange(1, n + 1)
    lab = lut[inv.reshape(-1)]
    first = np.stack(np.unravel_index(np.sort(at[keep]), raw.shape), axis=1).astype(np.int64).reshape(n, 3)
    size = np.bincount(lab, minlength=n + 1)[1:].astype(np.int64)
    bbox = np.zeros((n, 6), np.int64)
    if n:
        order = np.argsort(lab, kind="stable")
        order = order[len(lab) - int(size.sum()):]                    # the occupied voxels, grain by grain
        begin = np.concatenate(([0], np.cumsum(size)[:-1]))
        for a, c in enumerate(np.unravel_index(order, raw.shape)):
            bbox[:, a] = np.minimum.reduceat(c, begin)
            bbox[:, 3 + a] = np.maximum.reduceat(c, begin)
    return lab.reshape(raw.shape), first, size, bbox


KINDS = ("one", "stripes0", "stripes1", "stripes2", "blocks", "scattered", "constructed_blocks")


def _species(rs, occ):
    """states 1..4 drawn per occupied voxel, all four present when four voxels are occupied."""
    state = np.where(occ, rs.randint(1, 5, occ.shape), 0).astype(np.int64)
    if occ.sum() >= 4:
        state.reshape(-1)[rs.choice(np.flatnonzero(occ.reshape(-1)), 4, replace=False)] = np.arange(1, 5)
    return state


def one(L, seed=0):
    """the full lattice as one grain.  Returns raw, state."""
    raw = np.ones((L, L, L), np.int64)
    return raw, _species(np.random.RandomState(seed), raw != 0)


def stripes(L, a, w=3, seed=0):
    """grains are slabs of thickness w perpendicular to axis a, every 5th slab empty (3 and 5 share no factor with the
    kernel's tile edges 8, 32, 16: slab faces and tile faces meet in every relative position).  Returns raw, state."""
    slab = np.arange(L) // w
    line = np.where(slab % 5 == 4, 0, slab + 1)
    shape = [1, 1, 1]
    shape[a] = L
    raw = np.ascontiguousarray(np.broadcast_to(line.reshape(shape), (L, L, L))).astype(np.int64)
    return raw, _species(np.random.RandomState(seed), raw != 0)


def blocks(L, seed=0, fill=0.7):
    """the box partition of :func:`random_blocks` (edges 1..4 at random cuts) with ONE grain per filled box.  Returns raw,
    state."""
    rs = np.random.RandomState(seed)
    a, b, c, filled = _boxes(rs, L, fill)
    _, nb, nc = filled.shape
    box = (a[:, None, None] * nb + b[None, :, None]) * nc + c[None, None, :]
    raw = np.where(filled[np.ix_(a, b, c)], box + 1, 0).astype(np.int64)
    return raw, _species(rs, raw != 0)


def scattered(L, seed=0, fill=0.7, n_ids=3):
    """every voxel occupied with probability ``fill`` draws one of n_ids raw ids: the grains are disconnected, and the same,
    another and no label occur among the face neighbours in every combination.  Returns raw, state."""
    rs = np.random.RandomState(seed)
    occ = rs.random_sample((L, L, L)) < fill
    raw = np.where(occ, rs.randint(1, n_ids + 1, (L, L, L)), 0).astype(np.int64)
    return raw, _species(rs, occ)


def constructed_blocks(L, seed=0):
    """:func:`constructed` with every block one grain (:func:`block_labels`' labelling, as a raw volume): the only maker
    with both columnar and equiaxed grains.  Returns raw, state."""
    state, _, _, h = constructed(L, species=np.random.RandomState(seed))
    return (_block_key(L, h) + 1).astype(np.int64), state


# the shapes of the device comparison on imported labellings: every tile edge (8 rows, 32 columns, 16 planes) from both
# sides; 65 = two full column tiles and a remainder, five plane groups, a ragged last row tile
SHAPES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 34, 64, 65)


def case_seed(kind, L):
    """the fixed seed of the (kind, L) case: check_not_vacuous holds with it at every L of SHAPES (pinned on the host)."""
    return {"scattered": 196}.get(kind, 0) + L


def labelling(kind, L, seed=0):
    """raw, state of one of KINDS."""
    if kind.startswith("stripes"):
        return stripes(L, int(kind[-1]), seed=seed)
    return {"one": one, "blocks": blocks, "scattered": scattered, "constructed_blocks": constructed_blocks}[kind](L, seed)


# the kernel's block edges (csrc/layer.hpp: LAYER_TJ rows, LAYER_TK columns, LAYER_NI planes): (axis, last index before the edge)
EDGES = ((1, 7), (2, 31), (0, 15))


def straddles(labels, axis, at):
    """(same, other): is there a pair of occupied face neighbours across the edge between the indices at and at + 1 of
    ``axis`` with the same label / with two different labels."""
    lo = np.take(labels, at, axis=axis)
    hi = np.take(labels, at + 1, axis=axis)
    both = (lo != 0) & (hi != 0)
    return bool((both & (lo == hi)).any()), bool((both & (lo != hi)).any())


def check_not_vacuous(kind, L, labels, want):
    """Guards against a vacuous pass of a comparison on an imported labelling of KINDS (all but constructed_blocks, L >= 4),
    evaluated on the reference's inputs and result: the same-label side of every predicate is there, and same-label pairs
    lie across the kernel's tile, rim and plane-group edges.

    ``blocks`` is a product partition: across one edge its occupied pairs are ALL of one box or ALL of two, so it cannot
    have both sorts of pair at the same edge; there an occupied pair of either sort is asked for (test_layer_ref_host.py
    pins that over the shapes of the device test both sorts occur at every edge), while ``scattered`` has both at every
    edge of every shape."""
    if kind == "constructed_blocks" or L < 4:
        return
    n_occ, occ_s, gb_s = want["n_occ"].sum(), want["occ_state"].sum(), want["gb_state"].sum()
    assert n_occ > 0
    for a in range(3):
        assert want["seg"][:, a].sum() < n_occ, (kind, L, a)
    if kind in ("blocks", "scattered"):
        assert all(want["cut"][:, a].sum() > 0 for a in range(3)), (kind, L)
        assert 0 < gb_s < occ_s, (kind, L)
    if kind == "one":
        assert all(want["seg"][:, a].sum() == L * L for a in range(3))
        assert not want["cut"].any() and not want["gb_state"].any() and want["n_start"].sum() == 1
    for axis, at in EDGES:
        if L > at + 1:
            same, other = straddles(labels, axis, at)
            if kind == "blocks":
                assert same or other, (kind, L, axis)
            else:
                assert same, (kind, L, axis)
                if kind == "scattered":
                    assert other, (kind, L, axis)
