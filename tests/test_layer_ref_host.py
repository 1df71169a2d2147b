"""The NumPy comparator of the layer profile (layer_ref.py) and metrics.layer_metrics, pinned without a GPU: lattices whose
every counter is written out by hand, identities on random lattices, a constructed columnar / equiaxed lattice whose CET
plane is known, the empty and single-voxel lattices, and the labellings the device test imports (from_raw against the loop-based
block_labels, the makers, and the guards against a vacuous pass at every shape of that test)."""
import numpy as np
import pytest

import layer_ref as LR

AR = 3.0


def _tables(labels):
    """first voxel (row-major) and bounding box of the labels 1..n of a hand-written label volume."""
    n = int(labels.max())
    first, bbox = [], []
    for q in range(1, n + 1):
        at = np.argwhere(labels == q)
        first.append(at[0])
        bbox.append(list(at.min(axis=0)) + list(at.max(axis=0)))
    return np.array(first, np.int64).reshape(n, 3), np.array(bbox, np.int64).reshape(n, 6)


def _ref(labels, state, ar=AR):
    first, bbox = _tables(labels)
    return LR.layer_ref(labels, state, bbox, first, ar)


def test_hand_2():
    """2^3, every counter by hand.
        plane 0: [[1, 1], [2, 0]]     plane 1: [[1, 3], [2, 0]]        (rows j, columns k)
    grain 1 = (0,0,0) (0,0,1) (1,0,0): bbox 2 x 1 x 2, AR 2 -> equiaxed; grain 2 = (0,1,0) (1,1,0): 2 x 1 x 1, AR 2 ->
    equiaxed; grain 3 = (1,0,1): AR 1.  With ar_threshold 2.0 only grain 3 is equiaxed."""
    g = np.array([[[1, 1], [2, 0]], [[1, 3], [2, 0]]])
    s = np.array([[[1, 2], [3, 0]], [[4, 3], [3, 0]]])
    r = _ref(g, s)
    assert r["n_occ"].tolist() == [3, 3] and r["n_start"].tolist() == [2, 1] and r["n_eq"].tolist() == [3, 3]
    assert _ref(g, s, 2.0)["n_eq"].tolist() == [0, 1]
    # axis 0: plane 0 has no predecessor inside (3 segments start); plane 1: (1,0,0) continues 1, (1,0,1) is 3 over 1 (a
    # cut), (1,1,0) continues 2
    assert r["seg"][:, 0].tolist() == [3, 1] and r["cut"][:, 0].tolist() == [0, 1]
    # axis 1 (j): row 0 starts; (0,1,0) = 2 over 1: cut; (1,1,0) = 2 over 1: cut
    assert r["seg"][:, 1].tolist() == [3, 3] and r["cut"][:, 1].tolist() == [1, 1]
    # axis 2 (k): plane 0: (0,0,0) starts, (0,0,1) continues, (0,1,0) starts; plane 1: (1,0,0) starts, (1,0,1) = 3 after 1:
    # cut, (1,1,0) starts
    assert r["seg"][:, 2].tolist() == [2, 3] and r["cut"][:, 2].tolist() == [0, 1]
    assert r["occ_state"].tolist() == [[1, 1, 1, 0], [0, 0, 2, 1]]
    # boundary voxels: (0,0,0): j+1 is 2 -> yes; (0,0,1): j+1 empty -> yes; (0,1,0): j-1 is 1 -> yes; (1,0,0): k+1 is 3;
    # (1,0,1); (1,1,0): all six
    assert r["gb_state"].tolist() == [[1, 1, 1, 0], [0, 0, 2, 1]]


def test_hand_3():
    """3^3 with a boundary along each axis, an empty voxel between two grains (a segment start without a cut) and a voxel on
    every lattice face.  Planes (rows j, columns k):
        i = 0: [[1, 1, 1], [1, 1, 1], [0, 0, 0]]
        i = 1: [[2, 2, 0], [0, 0, 0], [3, 0, 4]]
        i = 2: [[2, 2, 0], [5, 5, 5], [3, 0, 4]]"""
    g = np.array([[[1, 1, 1], [1, 1, 1], [0, 0, 0]],
                  [[2, 2, 0], [0, 0, 0], [3, 0, 4]],
                  [[2, 2, 0], [5, 5, 5], [3, 0, 4]]])
    s = np.where(g != 0, 1, 0)
    s[0, 0, 0], s[0, 1, 1], s[2, 1, 1], s[1, 2, 2] = 2, 3, 4, 3
    r = _ref(g, s)
    assert r["n_occ"].tolist() == [6, 4, 7]
    assert r["n_start"].tolist() == [1, 3, 1]                 # grains 2, 3, 4 begin in plane 1, grain 5 in plane 2
    # bboxes: 1: 1x2x3 (AR 3: columnar at 3.0), 2: 2x1x2 (2), 3: 2x1x1 (2), 4: 2x1x1 (2), 5: 1x1x3 (3: columnar)
    assert r["n_eq"].tolist() == [0, 4, 4]
    # axis 0: plane 0 all start (6); plane 1: (1,0,0) (1,0,1) are 2 over 1: cuts; (1,2,0) (1,2,2) over empty: starts, no cut;
    # plane 2: 2, 2, 3, 4 continue; 5 5 5 over empty: three starts
    assert r["seg"][:, 0].tolist() == [6, 4, 3] and r["cut"][:, 0].tolist() == [0, 2, 0]
    # axis 1: plane 0: row 0 starts (3), row 1 continues; plane 1: 2 2 start (j = 0), 3 and 4 after empty: start;
    # plane 2: row 0 starts (2); row 1: 5 after 2, 5 after 2: cuts, 5 after empty: start; row 2: 3 after 5, 4 after 5: cuts
    assert r["seg"][:, 1].tolist() == [3, 4, 7] and r["cut"][:, 1].tolist() == [0, 0, 4]
    # axis 2: plane 0: one start per row (2); plane 1: 2 starts, 3 starts, 4 after the empty voxel: a start without a cut;
    # plane 2: 2 starts, 5 starts, 3 starts, 4 after empty starts
    assert r["seg"][:, 2].tolist() == [2, 3, 4] and r["cut"][:, 2].tolist() == [0, 0, 0]
    assert r["occ_state"].tolist() == [[4, 1, 1, 0], [3, 0, 1, 0], [6, 0, 0, 1]]
    # plane 0: every voxel of grain 1 sees plane 1 (2 or empty) or the empty row 2: all six are boundary voxels; planes 1
    # and 2 likewise (every voxel touches another label or an empty voxel)
    assert r["gb_state"].tolist() == r["occ_state"].tolist()
    assert np.all(r["cut"] <= r["seg"])


def test_interior_voxel_is_no_boundary():
    """one grain filling 3^3 but for one empty corner: the 3 face neighbours of the corner are boundary voxels, no other."""
    g = np.ones((3, 3, 3), np.int64)
    g[2, 2, 2] = 0
    r = _ref(g, np.where(g != 0, 3, 0))
    assert r["gb_state"][:, 2].tolist() == [0, 1, 2] and r["occ_state"][:, 2].tolist() == [9, 9, 8]
    assert r["seg"].tolist() == [[9, 3, 3], [0, 3, 3], [0, 3, 3]] and not r["cut"].any()
    assert r["n_start"].tolist() == [1, 0, 0]


@pytest.mark.parametrize("L,seed", [(6, 1), (9, 2), (12, 3)])
def test_identities_random(L, seed):
    import metrics
    state, theta, phi = LR.random_blocks(L, seed)
    labels, first, size, bbox = LR.host_clusters(state, theta, phi)
    r = LR.layer_ref(labels, state, bbox, first, AR)
    assert r["n_occ"].sum() == size.sum() == np.count_nonzero(state)
    assert r["n_start"].sum() == len(size)
    assert np.all(r["cut"] <= r["seg"]) and np.all(r["gb_state"] <= r["occ_state"])
    assert np.array_equal(r["occ_state"].sum(axis=1), r["n_occ"])
    for t in (2, 3):
        mask = state == t
        assert mask.any()
        assert r["gb_state"][:, t - 1].sum() / r["occ_state"][:, t - 1].sum() == metrics.compute_boundary_fraction(mask, labels)
    m = metrics.layer_metrics(r, L, 5e-6)
    assert m["GB_frac_C"] == metrics.compute_boundary_fraction(state == 3, labels)
    assert m["GB_frac_Re"] == metrics.compute_boundary_fraction(state == 2, labels)
    # the clustering's stencil has no face neighbours and keeps the parity of i + j + k: two face neighbours are never in
    # one grain, so with ITS labels every occupied voxel starts a segment on every axis
    assert np.array_equal(r["seg"], np.repeat(r["n_occ"][:, None], 3, axis=1))


def test_boundary_fraction_with_face_connected_labels():
    """The same identity where grains do have interiors (block labels): compute_boundary_fraction replicates the edge, i.e.
    ignores neighbours outside the lattice, as the definition does."""
    import metrics
    L, h = 10, 6
    rs = np.random.RandomState(4)
    state, _, _, _ = LR.constructed(L, h, species=rs)
    labels, first, bbox = LR.block_labels(L, h)
    labels[:h, 2:6, 2:6] = labels[0, 2, 2]                    # a 4 x 4 column: it has interior voxels
    _, at, inv = np.unique(labels.reshape(-1), return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(at[1:])) + 1                # renumbered 1.. by first voxel (label 0 stays 0)
    labels = np.concatenate(([0], order))[inv].reshape(labels.shape)
    first, bbox = _tables(labels)
    r = LR.layer_ref(labels, state, bbox, first, AR)
    for t in (1, 2, 3):
        got = r["gb_state"][:, t - 1].sum() / r["occ_state"][:, t - 1].sum()
        assert 0.0 < got < 1.0 and got == metrics.compute_boundary_fraction(state == t, labels)


@pytest.mark.parametrize("L,h", [(12, 7), (16, 7), (14, 9)])
def test_constructed_cet_plane(L, h):
    import metrics
    from constants import CET_AR_THRESHOLD
    assert (L - h - 1) % 2 == 0 and L % 2 == 0                # whole cubes only
    state, theta, phi, _ = LR.constructed(L, h)
    labels, first, bbox = LR.block_labels(L, h)
    r = LR.layer_ref(labels, state, bbox, first, CET_AR_THRESHOLD)
    m = metrics.layer_metrics(r, L, 5e-6)
    assert m["CET_plane"] == h + 1 and m["CET_height_um"] == (h + 1) * 5e-6 * 1e6
    assert m["InterceptRatio"] > 1.0
    n_cube = (L - h - 1) * L * L
    assert m["EqAreaFrac"] == n_cube / (n_cube + h * L * L)
    # mean intercepts: along the build direction one segment per column and per cube of every (j, k) line
    n_seg0 = L * L * (1 + (L - h - 1) // 2)
    assert m["Intercept_build_um"] == (n_cube + h * L * L) / n_seg0 * 5e-6 * 1e6
    assert m["Intercept_plane_um"] == 2.0 * 5e-6 * 1e6                                 # every in-plane segment is 2 voxels
    assert r["n_start"].tolist() == [(L // 2) ** 2 if (i == 0 or (i > h and (i - h - 1) % 2 == 0)) else 0 for i in range(L)]
    pl = m["planes"]
    assert pl["EqAreaFrac_i"].tolist() == [0.0] * (h + 1) + [1.0] * (L - h - 1) and len(pl["plane"]) == L
    # the engine's own grains (two per block, of the block's bounding box) give the same classes, hence the same CET plane
    hl, hf, hs, hb = LR.host_clusters(state, theta, phi)
    assert len(hs) == 2 * len(first)
    m2 = metrics.layer_metrics(LR.layer_ref(hl, state, hb, hf, CET_AR_THRESHOLD), L, 5e-6)
    assert m2["CET_plane"] == h + 1 and m2["EqAreaFrac"] == m["EqAreaFrac"] and m2["InterceptRatio"] == 1.0


def test_cet_plane_rule():
    import metrics

    def cet(n_occ, n_eq):
        L = len(n_occ)
        z3, z4 = np.zeros((L, 3), np.int64), np.zeros((L, 4), np.int64)
        return metrics.layer_metrics(dict(n_occ=n_occ, n_start=[0] * L, n_eq=n_eq, seg=z3, cut=z3, occ_state=z4, gb_state=z4),
                                     L, 5e-6)["CET_plane"]
    assert cet([4, 4, 4, 4], [0, 4, 1, 3]) == 3               # plane 2 is columnar: the run above it counts
    assert cet([4, 4, 0, 4], [0, 4, 0, 4]) == 1               # an empty plane neither breaks nor starts the run
    assert cet([4, 4, 4, 4], [4, 4, 4, 2]) == -1              # exactly the threshold (0.5) is not above it
    assert cet([4, 4, 0, 0], [3, 3, 0, 0]) == 0
    assert cet([0, 0, 0], [0, 0, 0]) == -1


def test_empty_and_single_voxel():
    import metrics
    for L in (1, 3):
        z = np.zeros((L, L, L), np.int64)
        r = LR.layer_ref(z, z, np.zeros((0, 6)), np.zeros((0, 3)), AR)
        assert all(not r[k].any() for k in LR.FIELDS)
        m = metrics.layer_metrics(r, L, 5e-6)
        assert m["CET_plane"] == -1 and m["CET_height_um"] == -1.0
        assert all(m[k] == 0.0 for k in metrics.LAYER_COLUMNS[2:])
    g = np.ones((1, 1, 1), np.int64)
    r = _ref(g, np.full((1, 1, 1), 3))
    assert r["n_occ"].tolist() == [1] and r["n_start"].tolist() == [1] and r["n_eq"].tolist() == [1]
    assert r["seg"].tolist() == [[1, 1, 1]] and r["cut"].tolist() == [[0, 0, 0]]
    assert r["occ_state"].tolist() == [[0, 0, 1, 0]] and r["gb_state"].tolist() == [[0, 0, 0, 0]]      # no neighbour inside
    m = metrics.layer_metrics(r, 1, 5e-6)
    assert m["CET_plane"] == 0 and m["CET_height_um"] == 0.0 and m["InterceptRatio"] == 1.0 and m["GB_frac_C"] == 0.0
    assert list(m)[:9] == list(metrics.LAYER_COLUMNS)


# ---- imported labellings: from_raw, the makers, the guards of tests/test_gpu_layer_imported.py ------------------------------
def test_from_raw_by_hand():
    raw = np.array([[[7, 7], [0, 2]], [[2, 9], [7, 0]]])
    lab, first, size, bbox = LR.from_raw(raw)
    assert lab.tolist() == [[[1, 1], [0, 2]], [[2, 3], [1, 0]]]
    assert first.tolist() == [[0, 0, 0], [0, 1, 1], [1, 0, 1]] and size.tolist() == [3, 2, 1]
    assert bbox.tolist() == [[0, 0, 0, 1, 1, 1], [0, 0, 0, 1, 1, 1], [1, 0, 1, 1, 0, 1]]
    lab, first, size, bbox = LR.from_raw(np.zeros((3, 3, 3), np.int64))
    assert not lab.any() and first.shape == (0, 3) and size.shape == (0,) and bbox.shape == (0, 6)


@pytest.mark.parametrize("L", (5, 8, 9))
def test_from_raw_against_block_labels(L):
    state, _, _, h = LR.constructed(L)
    labels, first, bbox = LR.block_labels(L, h)
    raw, _ = LR.constructed_blocks(L)
    lab, f, size, b = LR.from_raw(raw * 3 + 11 * (raw != 0))             # any other raw ids of the same partition
    assert np.array_equal(lab, labels) and np.array_equal(f, first) and np.array_equal(b, bbox)
    assert np.array_equal(size, np.bincount(labels.reshape(-1))[1:]) and np.array_equal(lab != 0, state != 0)
    t_first, t_bbox = _tables(labels)
    assert np.array_equal(f, t_first) and np.array_equal(b, t_bbox)


@pytest.mark.parametrize("kind", LR.KINDS)
def test_makers_and_guards(kind):
    """every (kind, L) case of the device test: an importable labelling (ids 1..n by first occurrence), all four species,
    and the guards against a vacuous pass hold with the fixed seeds."""
    sorts = {}
    for L in LR.SHAPES:
        raw, state = LR.labelling(kind, L, LR.case_seed(kind, L))
        assert raw.shape == state.shape == (L, L, L) and np.array_equal(raw != 0, state != 0)
        lab, first, size, bbox = LR.from_raw(raw)
        n = len(size)
        seen = lab.reshape(-1)[np.sort(np.unique(lab.reshape(-1), return_index=True)[1])]
        assert seen[seen != 0].tolist() == list(range(1, n + 1))
        assert np.array_equal(lab != 0, raw != 0) and size.sum() == np.count_nonzero(raw)
        for q in [q for q in {1, (n + 1) // 2, n} if 1 <= q <= n]:       # spot checks against the plain definition
            at = np.argwhere(lab == q)
            assert len(at) == size[q - 1] and at[0].tolist() == first[q - 1].tolist() and len(np.unique(raw[lab == q])) == 1
            assert bbox[q - 1].tolist() == list(at.min(axis=0)) + list(at.max(axis=0))
        if L >= 3:
            assert set(np.unique(state)) - {0} == {1, 2, 3, 4}, (kind, L)
        want = LR.layer_ref(lab, state, bbox, first, AR)
        LR.check_not_vacuous(kind, L, lab, want)
        for axis, at in LR.EDGES:
            if L > at + 1:
                same, other = LR.straddles(lab, axis, at)
                sorts.setdefault(axis, set()).update({"same"} if same else set(), {"other"} if other else set())
    if kind in ("blocks", "scattered"):
        assert all(sorts[a] == {"same", "other"} for a in range(3)), sorts
    if kind == "scattered":
        assert np.unique(raw).tolist() == [0, 1, 2, 3]                  # of the last, largest shape


def test_makers_by_hand():
    raw, _ = LR.stripes(17, 1)
    assert raw[0, :, 0].tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 0, 0, 0, 6, 6] and (raw == raw[:1, :, :1]).all()
    assert (LR.one(4)[0] == 1).all()
    lab, _, size, bbox = LR.from_raw(LR.blocks(12, 3)[0])
    ext = bbox[:, 3:] - bbox[:, :3] + 1
    assert np.array_equal(size, ext.prod(axis=1)) and ext.max() <= 4          # one filled box = one grain


def test_guards_catch_a_parity_labelling():
    """the device clustering's own kind of labelling (no two face neighbours in one grain) fails the guards."""
    L = 9
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    lab, first, size, bbox = LR.from_raw(1 + (i + j + k) % 2)
    want = LR.layer_ref(lab, np.where(lab != 0, 1, 0), bbox, first, AR)
    with pytest.raises(AssertionError):
        LR.check_not_vacuous("scattered", L, lab, want)
