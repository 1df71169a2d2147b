"""The NumPy comparator of the texture profile (texture_ref.py) pinned on hand-computed lattices, its binning rule at values
exactly on an edge, the two identities with the layer profile's comparator, metrics.texture_metrics on a constructed
profile, the inputs of the device tests (no near-edge value, no vacuous labelling) and the binding's new entries.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import layer_ref as LR
import texture_ref as TR


def _lab(raw):
    return LR.from_raw(np.asarray(raw, np.int64))


def test_binning_rule_on_the_edges():
    """bin(x) = number of edges with x <= e[q]: a value equal to an edge belongs to the bin BELOW that edge's cosine (the
    larger angle side), bin 0 holds everything above e[0], the last bin everything at or below the last edge."""
    e = np.array([0.5, 0.0, -0.5])
    assert TR.bin_of(np.array([1.0 + 1e-15, 1.0, 0.75, 0.5, 0.25, 0.0, -0.25, -0.5, -1.0]), e).tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3]
    assert TR.bin_of(np.array([np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0)]), e).tolist() == [0, 1]
    assert TR.bin_of(np.array([0.3, -7.0]), np.zeros(0)).tolist() == [0, 0]          # n_bins == 1: no edge
    assert TR.ambiguous(np.array([0.5 + 5e-13, 0.5 + 5e-12, np.nan, -0.5]), e) == 2
    assert TR.ambiguous(np.array([0.25, 0.75]), e) == 0
    c = TR.edges_cos(36, 180.0)
    assert len(c) == 35 and (np.diff(c) < 0).all() and abs(c[17]) < 1e-15


def test_bicrystal_with_known_angle():
    """2^3: plane 0 is grain 1 along +z (theta 0), plane 1 grain 2 tilted by 60 degrees in the x-z plane: the four faces
    across axis 0 have d = cos 60 = 0.5 (up to rounding: below edge 0.75, above 0.25), no face across axes 1 and 2."""
    raw = np.zeros((2, 2, 2), np.int64)
    raw[0], raw[1] = 1, 2
    theta = np.where(raw == 2, np.pi / 3, 0.0)
    phi = np.zeros((2, 2, 2))
    e = np.array([0.75, 0.25, -0.25])
    got = TR.texture_ref(raw, theta, phi, e, np.array([0.9, 0.6, 0.3]), axis=(0.0, 0.0, 1.0))
    want_gb = np.zeros((2, 3, 4), np.int64)
    want_gb[1, 0, 1] = 4
    assert np.array_equal(got["gb_hist"], want_gb)
    # pole against z: plane 0 has c = 1 (bin 0), plane 1 c = cos 60 = 0.5 (0.6 >= c > 0.3: bin 2)
    assert got["pole_hist"].tolist() == [[4, 0, 0, 0], [0, 0, 4, 0]]
    assert not got["bad"].any()
    # the same crystal with the grains side by side along axis 2
    got = TR.texture_ref(raw.transpose(2, 1, 0), theta.transpose(2, 1, 0), phi, e, np.array([0.9, 0.6, 0.3]), axis=(0.0, 0.0, 1.0))
    assert got["gb_hist"][:, 2, 1].tolist() == [2, 2] and got["gb_hist"].sum() == 4


def test_identical_orientations_under_different_labels():
    """3^3 scattered labels, one orientation everywhere: every face has d = |o|^2 = 1 within rounding -> bin 0."""
    raw, _ = LR.scattered(3, seed=5, fill=0.9)
    lab, first, _, bbox = _lab(raw)
    theta, phi = np.full(raw.shape, 0.7), np.full(raw.shape, 2.1)
    e = TR.edges_cos(16, 180.0)
    got = TR.texture_ref(lab, theta, phi, e, TR.edges_cos(16, 90.0))
    assert got["gb_hist"].sum() > 0 and got["gb_hist"][:, :, 1:].sum() == 0 and not got["bad"].any()
    want = LR.layer_ref(lab, np.where(lab != 0, 1, 0), bbox, first, 3.0)
    assert np.array_equal(got["gb_hist"][:, :, 0], want["cut"])


def test_nan_theta_goes_to_bad():
    """3^3 full lattice of 27 one-voxel grains, theta NaN at the centre: its three predecessor faces, the three faces of its
    successors and its pole value are bad and in no bin."""
    lab = np.arange(1, 28, dtype=np.int64).reshape(3, 3, 3)
    theta, phi = TR.random_angles(3)
    theta[1, 1, 1] = np.nan
    e, pe = TR.edges_cos(4, 180.0), TR.edges_cos(4, 90.0)
    got = TR.texture_ref(lab, theta, phi, e, pe)
    want_bad = np.zeros((3, 4), np.int64)
    want_bad[1] = [1, 1, 1, 1]            # the centre's own faces and pole value, in its plane 1
    want_bad[2, 0] = 1                    # (2, 1, 1) across axis 0
    want_bad[1, 1] += 1                   # (1, 2, 1) across axis 1
    want_bad[1, 2] += 1                   # (1, 1, 2) across axis 2
    assert np.array_equal(got["bad"], want_bad)
    assert got["gb_hist"].sum() == 3 * 18 - 6 and got["pole_hist"].sum() == 26
    phi[0, 0, 0] = np.inf
    assert TR.texture_ref(lab, theta, phi, e, pe)["bad"][0].tolist() == [0, 1, 1, 1]


@pytest.mark.parametrize("kind", TR.KINDS)
@pytest.mark.parametrize("L", (5, 9, 17, 33))
def test_identities_with_the_layer_comparator(L, kind):
    """sum_b gb_hist + bad == cut and sum_b pole_hist + bad[3] == n_occ of layer_ref on the same labelling."""
    lab = TR.labelling(kind, L)
    _, first, _, bbox = LR.from_raw(lab)
    theta, phi = TR.random_angles(L)
    theta[0, 0, :] = np.nan
    layer = LR.layer_ref(lab, np.where(lab != 0, 1, 0), bbox, first, 3.0)
    for nb in (1, 16):
        got = TR.texture_ref(lab, theta, phi, TR.edges_cos(nb, 180.0), TR.edges_cos(nb, 90.0), axis=(0.2, -1.0, 0.4))
        assert np.array_equal(got["gb_hist"].sum(axis=2) + got["bad"][:, :3], layer["cut"])
        assert np.array_equal(got["pole_hist"].sum(axis=1) + got["bad"][:, 3], layer["n_occ"])
    assert layer["cut"].sum() > 0 and got["bad"].sum() > 0


def test_device_test_inputs():
    """What the device tests rely on, checked where it costs no GPU time: over their shapes and bin counts no value of the
    random orientations lies within the guard of an edge -- on EVERY face, a superset of the grain-grain faces of any
    labelling -- and the labellings put both sorts of predecessor across the kernel's block edges."""
    for L in (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65):
        theta, phi = TR.random_angles(L)
        every = np.arange(1, L ** 3 + 1).reshape(L, L, L)          # every face is a grain-grain face
        for axis in ((1.0, 0.0, 0.0), (1.0, 2.0, -2.0)):
            values = (TR.face_values(every, theta, phi), TR.pole_values(every, theta, phi, axis))
            for nb in (1, 2, 16, 64):
                assert TR.n_ambiguous(values, TR.edges_cos(nb, 180.0), TR.edges_cos(nb, 90.0)) == 0, (L, nb, axis)
        for kind in TR.KINDS:
            TR.check_not_vacuous(kind, L, TR.labelling(kind, L))


def test_texture_metrics_columns():
    import metrics
    L, nb = 2, 36
    gb, pole, bad = np.zeros((L, 3, nb), np.int64), np.zeros((L, nb), np.int64), np.zeros((L, 4), np.int64)
    gb[0, 0, 0] = 2          # 0..5 degrees across the build axis: centre 2.5
    gb[0, 1, 2] = 1          # 10..15 degrees, lateral: centre 12.5
    gb[1, 2, 3] = 1          # 15..20 degrees, lateral: centre 17.5, not low-angle
    gb[1, 0, 35] = 4         # 175..180 degrees: centre 177.5
    pole[0, 1], pole[0, 17], pole[1, 2], pole[1, 3] = 3, 1, 2, 2     # 2.5 degree steps: bins 0..5 end at or below 15
    pole[1, 6] = 2
    bad[1] = [0, 1, 0, 2]
    prof = dict(gb_hist=gb, pole_hist=pole, bad=bad, gb_edges_deg=np.arange(1, nb) * 5.0, pole_edges_deg=np.arange(1, nb) * 2.5)
    m = metrics.texture_metrics(prof)
    assert tuple(k for k in m if k != "planes") == metrics.TEXTURE_COLUMNS
    assert m["GB_faces"] == 8 and m["Texture_bad"] == 3
    assert m["GB_misorientation_mean_deg"] == pytest.approx((2 * 2.5 + 12.5 + 17.5 + 4 * 177.5) / 8, rel=1e-12)
    assert m["GB_low_angle_frac"] == 3 / 8 and m["GB_lateral_frac"] == 2 / 8 and m["Pole_aligned_frac"] == 7 / 10
    p = m["planes"]
    assert p["plane"].tolist() == [0, 1] and p["GB_faces"].tolist() == [3, 5] and p["GB_low_angle_frac"].tolist() == [1.0, 0.0]
    assert p["GB_faces0"].tolist() == [2, 4] and p["bad3"].tolist() == [0, 2] and p["gb1_bin2"].tolist() == [1, 0]
    assert p["Pole_aligned_frac"].tolist() == [0.75, 4 / 6]
    empty = metrics.texture_metrics(dict(prof, gb_hist=gb * 0, pole_hist=pole * 0, bad=bad * 0))
    assert [empty[c] for c in metrics.TEXTURE_COLUMNS] == [0, 0.0, 0.0, 0.0, 0.0, 0]


def test_write_texture_csv(tmp_path):
    import metrics
    import pandas as pd
    lab = TR.labelling("checker", 5)
    theta, phi = TR.random_angles(5)
    prof = TR.texture_ref(lab, theta, phi, TR.edges_cos(4, 180.0), TR.edges_cos(4, 90.0))
    prof.update(gb_edges_deg=np.arange(1, 4) * 45.0, pole_edges_deg=np.arange(1, 4) * 22.5)
    planes = metrics.texture_metrics(prof)["planes"]
    metrics.write_texture_csv(str(tmp_path / "texture.csv"), planes)
    df = pd.read_csv(tmp_path / "texture.csv")
    assert len(df) == 5 and list(df.columns) == list(planes)
    assert df["gb0_bin1"].tolist() == prof["gb_hist"][:, 0, 1].tolist() and df["pole_bin3"].tolist() == prof["pole_hist"][:, 3].tolist()


def test_binding_names_the_new_entries():
    from cetkmc import _lib
    for name in ("cetkmc_texture_profile", "cetkmc_ensemble_texture_profile"):
        assert name in _lib.PROTOTYPES
        assert _lib.PROTOTYPES[name][1][1] == C.POINTER(_lib.TextureArgs)
    assert _lib.STRUCT_MIRRORS["texture_args"] is _lib.TextureArgs
    assert C.sizeof(_lib.TextureArgs) == 48 and _lib.TextureArgs.axis.offset == 24


def test_default_edges_of_the_engine():
    """Engine.texture_profile's default edges: equal steps, the 5-degree boundary edges contain 15 degrees exactly, and their
    cosines are the comparator's."""
    from cetkmc import engine
    a, keep, gb_deg, pole_deg = engine._texture_args(36, None, None, (1.0, 0.0, 0.0))
    assert gb_deg.tolist() == [5.0 * q for q in range(1, 36)] and pole_deg.tolist() == [2.5 * q for q in range(1, 36)]
    assert np.array_equal(keep[0], TR.edges_cos(36, 180.0)) and np.array_equal(keep[1], TR.edges_cos(36, 90.0))
    assert a.n_bins == 36 and list(a.axis) == [1.0, 0.0, 0.0]
    a, keep, _, _ = engine._texture_args(1, None, None, (0.0, 1.0, 0.0))
    assert a.n_bins == 1 and not a.gb_edges and not a.pole_edges
    with pytest.raises(ValueError, match="interior edges"):
        engine._texture_args(4, [10.0], None, (1.0, 0.0, 0.0))
