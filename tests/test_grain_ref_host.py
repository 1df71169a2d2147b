"""The NumPy comparator of the per-grain table (grain_ref.py) pinned without a GPU: hand-computed 2^3 and 3^3 lattices with
every counter written out, the identities of the definition on random labellings and against layer_ref.py, the columns of
metrics.grain_metrics on grains whose moments are known in closed form, and the guards of every input the GPU files use."""
import numpy as np
import pytest

import cluster_ref as CR
import grain_ref as GR
import layer_ref as LR


def _table(voxel_lists, L=None, theta=None, phi=None):
    """the comparator's table of grains given as lists of voxels (numbered by first voxel, as an import demands)"""
    L = L or 1 + max(max(v) for vs in voxel_lists for v in vs)
    raw = np.zeros((L, L, L), np.int64)
    for q, vs in enumerate(voxel_lists):
        for v in vs:
            raw[tuple(v)] = q + 1
    lab = LR.from_raw(raw)[0]
    z = np.zeros((L, L, L))
    return GR.grain_ref(lab, (lab != 0).astype(np.int64), z if theta is None else theta, z if phi is None else phi), lab


def test_hand_2():
    """2^3: every +-2 offset leaves the lattice and of each group of four diagonal offsets exactly one stays inside, so a
    voxel (i, j, k) has the two neighbours A = (1-i, 1-j, k) and B = (i, 1-j, 1-k) and 12 contacts outside."""
    lab = np.array([1, 0, 2, 3, 2, 1, 0, 3]).reshape(2, 2, 2)
    state = np.array([1, 0, 2, 3, 4, 0, 0, 1]).reshape(2, 2, 2)
    theta, phi = (np.arange(8) * 0.1).reshape(2, 2, 2), (1.0 + np.arange(8) * 0.2).reshape(2, 2, 2)
    t = GR.grain_ref(lab, state, theta, phi)
    # grain 1 = {000, 101}: 000 -> A 110 empty, B 011 other; 101 -> A 011 other, B 110 empty.  101 has state 0: in no species
    # grain 2 = {010, 100}: 010 -> A 100 same, B 001 empty; 100 -> A 010 same, B 111 other
    # grain 3 = {011, 111}: 011 -> A 101 other, B 000 other; 111 -> A 001 empty, B 100 other
    assert t["n"].tolist() == [2, 2, 2]
    assert t["sum"].tolist() == [[1, 0, 1], [1, 1, 0], [1, 2, 2]]
    assert t["sq"].tolist() == [[1, 0, 1, 0, 1, 0], [1, 1, 0, 0, 0, 0], [1, 2, 2, 1, 1, 2]]
    assert t["n_state"].tolist() == [[1, 0, 0, 0], [0, 1, 0, 1], [1, 0, 1, 0]]
    assert t["nb"].tolist() == [[0, 2, 2, 24], [2, 1, 1, 24], [0, 3, 1, 24]]
    assert t["first_theta"].tolist() == [theta[0, 0, 0], theta[0, 1, 0], theta[0, 1, 1]]
    assert t["first_phi"].tolist() == [phi[0, 0, 0], phi[0, 1, 0], phi[0, 1, 1]]
    assert all(t[k].dtype == np.int64 for k in GR.INT_FIELDS)
    GR.check_identities(t)


def test_hand_3():
    """3^3.  One grain: per coordinate 9 * (0 + 1 + 2) = 27, squares 9 * (0 + 1 + 4) = 45, products 3 * 3 * 3 = 27; a
    diagonal offset stays inside for 2 * 2 * 3 = 12 voxels (8 offsets), a +-2 offset for 9 (6 offsets): 150 contacts inside,
    14 * 27 - 150 = 228 outside.  Then the centre as grain 2 (8 diagonal neighbours, 6 outside) and the corner (2, 2, 2)
    empty (5 neighbours inside: (1,1,2), (2,1,1), (0,2,2), (2,0,2), (2,2,0); none is the centre)."""
    z = np.zeros((3, 3, 3))
    one = GR.grain_ref(np.ones((3, 3, 3), np.int64), np.full((3, 3, 3), 2), z, z)
    assert one["n"].tolist() == [27] and one["sum"].tolist() == [[27, 27, 27]]
    assert one["sq"].tolist() == [[45, 45, 45, 27, 27, 27]]
    assert one["n_state"].tolist() == [[0, 27, 0, 0]] and one["nb"].tolist() == [[150, 0, 0, 228]]
    lab = np.ones((3, 3, 3), np.int64)
    lab[1, 1, 1], lab[2, 2, 2] = 2, 0
    state = np.where(lab == 2, 3, 1)
    t = GR.grain_ref(lab, state, z + 0.5, z + 0.25)
    # grain 1: 150 - 8 (from the centre) - 5 (from the corner) = 137 contacts inside, 8 of them to the centre, 5 to the
    # corner; outside 228 - 6 (centre) - 9 (corner)
    assert t["n"].tolist() == [25, 1]
    assert t["sum"].tolist() == [[24, 24, 24], [1, 1, 1]]
    assert t["sq"].tolist() == [[40, 40, 40, 22, 22, 22], [1, 1, 1, 1, 1, 1]]
    assert t["n_state"].tolist() == [[25, 0, 0, 0], [0, 0, 1, 0]]          # the corner carries state 1 but no label: in none
    assert t["nb"].tolist() == [[124, 8, 5, 213], [0, 8, 0, 6]]
    assert t["first_theta"].tolist() == [0.5, 0.5] and t["first_phi"].tolist() == [0.25, 0.25]
    GR.check_identities(t)


def test_angles_are_copied_bitwise():
    nan2 = np.array([0x7ff8000000000123], dtype=np.int64).view(np.float64)[0]       # a NaN with a payload
    th = np.array([nan2, 1.0, -np.inf, 2.0, 0.0, 0.0, 0.0, -0.0]).reshape(2, 2, 2)
    lab = np.array([1, 1, 2, 0, 3, 0, 0, 4]).reshape(2, 2, 2)
    t = GR.grain_ref(lab, lab, th, th[::-1].copy())
    assert t["first_theta"].view(np.int64).tolist() == th.reshape(-1)[[0, 2, 4, 7]].view(np.int64).tolist()
    assert GR.same(t, t) == []
    u = {k: v.copy() for k, v in t.items()}
    u["first_theta"][3] = 0.0                                                      # +0.0 against -0.0: other bits
    assert GR.same(u, t) == ["first_theta"]
    u = {k: v.copy() for k, v in t.items()}
    u["nb"][1, 2] += 1
    assert GR.same(u, t) == ["nb"]


@pytest.mark.parametrize("L,seed", [(5, 1), (9, 2), (16, 3)])
def test_identities_random(L, seed):
    rs = np.random.RandomState(seed)
    raw = np.where(rs.random_sample((L, L, L)) < 0.7, rs.randint(1, 9, (L, L, L)), 0)
    lab, first, size, bbox = LR.from_raw(raw)
    state = rs.randint(0, 6, (L, L, L))                    # labelled voxels with the states 0 and 5 too
    th, ph = GR.angles(L, seed)
    t = GR.grain_ref(lab, state, th, ph)
    GR.check_identities(t, size, LR.layer_ref(lab, state, bbox, first, 3.0))
    assert (t["n_state"].sum(axis=1) < t["n"]).any()
    at = first[:, 0] * L * L + first[:, 1] * L + first[:, 2]
    assert GR.same(dict(t, first_theta=th.reshape(-1)[at], first_phi=ph.reshape(-1)[at]), t) == []
    # a second way to the contact counts: every ordered pair of the stencil, one offset at a time
    nb = np.zeros_like(t["nb"])
    for v in np.argwhere(lab > 0).tolist():
        for d in GR.STENCIL:
            u = [a + b for a, b in zip(v, d)]
            g = lab[tuple(v)]
            c = 3 if min(u) < 0 or max(u) >= L else (2 if lab[tuple(u)] == 0 else (0 if lab[tuple(u)] == g else 1))
            nb[g - 1, c] += 1
    assert np.array_equal(nb, t["nb"])


def test_pinned_inputs():
    """what the issue records of two inputs of the GPU tests"""
    state, theta, phi = CR.continuous(33, 0.6, 33)
    ref = CR.cluster_ref(state, theta, phi, 0.9)
    t = GR.grain_ref(ref["labels"], state, theta, phi)
    GR.check_identities(t, ref["size"])
    GR.check_clustered(t, largest=0.10)
    assert len(t["n"]) == 5989 and int((t["n"] > 1).sum()) == 1922
    assert 0.165 < t["n"].max() / t["n"].sum() < 0.175
    assert t["nb"].sum(axis=0).tolist() == [58886, 111144, 113654, 18366]
    state, theta, phi = CR.textured()
    ref = CR.cluster_ref(state, theta, phi, 0.5)
    t = GR.grain_ref(ref["labels"], state, theta, phi)
    GR.check_clustered(t, largest=0.10)
    assert len(t["n"]) == 3 and 0.49 < t["n"].max() / t["n"].sum() < 0.51


@pytest.mark.parametrize("L", GR.SHAPES)
def test_imported_inputs(L):
    """every imported labelling of test_gpu_grain_table.py: same-label stencil pairs across every edge of the kernel"""
    for kind in LR.KINDS:
        raw, state = LR.labelling(kind, L, LR.case_seed(kind, L))
        lab = LR.from_raw(raw)[0]
        th, ph = GR.angles(L, L)
        t = GR.grain_ref(lab, state, th, ph)
        GR.check_identities(t, LR.from_raw(raw)[2])
        GR.check_import(kind, L, lab, t)


def test_regime_inputs():
    lab, state = GR.singletons(65)
    n = int((lab > 0).sum())
    assert n > 65 ** 3 // 2 and np.array_equal(lab.reshape(-1)[lab.reshape(-1) > 0], np.arange(1, n + 1))
    assert n > 100 * GR.SLOTS                                  # far more labels in a block than its table has slots
    raw, state = LR.one(129)
    assert LR.from_raw(raw)[0].min() == 1
    L = 9
    lab = LR.from_raw(LR.labelling("scattered", L, LR.case_seed("scattered", L))[0])[0]
    state = np.where(lab > 0, np.arange(L ** 3).reshape(L, L, L) % 5, 0)
    t = GR.grain_ref(lab, state, np.zeros((L, L, L)), np.zeros((L, L, L)))
    assert (t["n_state"].sum(axis=1) < t["n"]).all()


@pytest.mark.parametrize("name", sorted(CR.ENSEMBLES))
def test_ensemble_inputs(name):
    L, thresholds = CR.ENSEMBLES[name]
    for r, (st, th, ph, _) in enumerate(CR.ensemble_lattices(name)):
        ref = CR.cluster_ref(st, th, ph, thresholds[0])
        t = GR.grain_ref(ref["labels"], st, th, ph)
        GR.check_identities(t, ref["size"])
        if name == "L30_R6" and r == 2:
            assert len(t["n"]) == 0
        elif name == "L30_R6" and r == 3:
            assert (t["n"] == 1).all() and not t["nb"][:, :2].any()
        else:
            GR.check_clustered(t, full=(name == "L30_R6" and r == 1))


# ---- metrics.grain_metrics --------------------------------------------------------------------------------------------------
def _close(a, b):
    return abs(a - b) <= 1e-9 * max(abs(b), 1.0)


def _box(lo, ext):
    return [(lo[0] + a, lo[1] + b, lo[2] + c) for a in range(ext[0]) for b in range(ext[1]) for c in range(ext[2])]


def test_metrics_boxes_and_rods():
    import constants as K
    import metrics
    assert metrics.GRAIN_COLUMNS == ("Grain_elong_mean", "Columnar_vol_frac", "Grain_incl_mean_deg", "Largest_grain_frac",
                                     "Contact_same_frac", "Aligned_vol_frac")
    assert float(K.CET_AR_THRESHOLD) <= 5.0
    # a 2 x 2 x 12 box along axis 0: variances 143/12 + 1/12 = 12, 3/12 + 1/12 = 1/3 twice: elong sqrt(36) = 6, incl 0
    m = metrics.grain_metrics(_table([_box((0, 0, 0), (12, 2, 2))])[0])
    g = m["grains"]
    assert _close(g["elong"][0], 6.0) and abs(g["incl_deg"][0]) <= 1e-9
    assert _close(g["len_major"][0], 12.0) and _close(g["len_mid"][0], 2.0) and _close(g["len_minor"][0], 2.0)
    assert _close(g["ci"][0], 5.5) and _close(g["cj"][0], 0.5) and _close(g["ck"][0], 0.5)
    assert m["Columnar_vol_frac"] == 1.0 and _close(m["Grain_elong_mean"], 6.0) and m["Largest_grain_frac"] == 1.0
    assert abs(m["Grain_incl_mean_deg"]) <= 1e-9
    # the same box along axis 2: incl 90, not columnar
    m = metrics.grain_metrics(_table([_box((0, 0, 0), (2, 2, 12))])[0])
    assert _close(m["grains"]["elong"][0], 6.0) and abs(m["grains"]["incl_deg"][0] - 90.0) <= 1e-9
    assert m["Columnar_vol_frac"] == 0.0 and abs(m["Grain_incl_mean_deg"] - 90.0) <= 1e-9
    # the rod (t, t, 0), t = 0..4: variance 2 along i and j with covariance 2, so 4 + 1/12 along (1, 1, 0), 1/12 across:
    # elong sqrt(49) = 7, incl 45
    m = metrics.grain_metrics(_table([[(t, t, 0) for t in range(5)]])[0])
    assert _close(m["grains"]["elong"][0], 7.0) and abs(m["grains"]["incl_deg"][0] - 45.0) <= 1e-9
    # a single voxel: isotropic
    m = metrics.grain_metrics(_table([[(3, 1, 2)]])[0])
    assert _close(m["grains"]["elong"][0], 1.0) and _close(m["grains"]["len_major"][0], 1.0)
    assert m["Columnar_vol_frac"] == 0.0 and m["Grain_incl_mean_deg"] == 0.0      # no grain is elongated: the mean is 0.0


def test_metrics_cubic_box_rod():
    """the rod (t, t, t), t = 0..2, has a cubic bounding box -- equiaxed by the bounding-box rule -- but variance 2 + 1/12
    along (1, 1, 1) and 1/12 across: elong 5, inclined by acos(1 / sqrt 3) = 54.74 degrees, so elongated but not columnar;
    the 2 x 2 x 12 box beside it is."""
    import metrics
    t, lab = _table([_box((0, 0, 0), (12, 2, 2)), [(3 + q, 4 + q, 4 + q) for q in range(3)]])
    bbox = LR.from_raw(lab)[3]
    assert (bbox[1, 3:] - bbox[1, :3]).tolist() == [2, 2, 2]
    m = metrics.grain_metrics(t)
    g = m["grains"]
    assert _close(g["elong"][1], 5.0) and abs(g["incl_deg"][1] - np.degrees(np.arccos(1.0 / np.sqrt(3.0)))) <= 1e-9
    assert _close(m["Columnar_vol_frac"], 48.0 / 51.0)
    assert _close(m["Grain_elong_mean"], (48.0 * 6.0 + 3.0 * 5.0) / 51.0)
    assert abs(m["Grain_incl_mean_deg"] - 3.0 * g["incl_deg"][1] / 51.0) <= 1e-9
    assert _close(m["Largest_grain_frac"], 48.0 / 51.0)
    # the mirrored rod (t, 2 - t, t) has the same inclination
    m2 = metrics.grain_metrics(_table([[(q, 2 - q, q) for q in range(3)]])[0])
    assert abs(m2["grains"]["incl_deg"][0] - g["incl_deg"][1]) <= 1e-9


def test_metrics_contacts_alignment_and_empty(tmp_path):
    import metrics
    L = 4
    th, ph = np.zeros((L, L, L)), np.zeros((L, L, L))
    # grain 1 starts at (0, 0, 0): vector (1, 0, 0), aligned; grain 2 at (0, 0, 2): 10 degrees off the opposite direction,
    # aligned; grain 3 at (2, 0, 0): 20 degrees off, not; grain 4 at (2, 2, 2): NaN, not
    th[0, 0, 0], ph[0, 0, 0] = np.pi / 2, 0.0
    th[0, 0, 2], ph[0, 0, 2] = np.pi / 2, np.pi + np.radians(10.0)
    th[2, 0, 0], ph[2, 0, 0] = np.pi / 2 - np.radians(20.0), 0.0
    th[2, 2, 2] = np.nan
    t, lab = _table([_box((0, 0, 0), (2, 4, 2)), _box((0, 0, 2), (2, 4, 2)), _box((2, 0, 0), (2, 2, 4)), [(2, 2, 2)]], L, th, ph)
    assert t["n"].tolist() == [16, 16, 16, 1]
    m = metrics.grain_metrics(t)
    assert _close(m["Aligned_vol_frac"], 32.0 / 49.0)
    same, other = int(t["nb"][:, 0].sum()), int(t["nb"][:, 1].sum())
    assert same > 0 and other > 0 and m["Contact_same_frac"] == same / (same + other)
    assert m["grains"]["id"].tolist() == [1, 2, 3, 4] and m["grains"]["nb_same"].tolist() == t["nb"][:, 0].tolist()
    assert m["grains"]["n_W"].tolist() == [16, 16, 16, 1]
    metrics.write_grains_csv(tmp_path / "g.csv", m["grains"])
    rows = (tmp_path / "g.csv").read_text().strip().splitlines()
    assert len(rows) == 5 and rows[0].split(",")[:3] == ["id", "n", "ci"] and rows[4].split(",")[:2] == ["4", "1"]
    empty = metrics.grain_metrics(GR.grain_ref(np.zeros((3, 3, 3), np.int64), np.zeros((3, 3, 3)), th[:3, :3, :3], ph[:3, :3, :3]))
    assert [empty[c] for c in metrics.GRAIN_COLUMNS] == [0.0] * 6 and len(empty["grains"]["id"]) == 0
