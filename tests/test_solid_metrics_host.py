"""metrics.solid_metrics and cetkmc.engine.default_solid_scales pinned without a GPU, on numbers written out by hand: the
eight columns, the planes table and the grains table of a hand-written profile (known n_rec, q, stamps and bad voxels, an
empty plane, a grain without a record, a clustering beside it), the Gi = 0 case, and the physical units of the default
scales: a known temperature step per voxel edge must come back in K/m and a known change per microsecond in K/s."""
import csv

import numpy as np

import solid_ref as SR

I64MAX = np.iinfo(np.int64).max
SCALES = (4.0, 2.0, 0.5, 8.0)          # powers of two: every mean below is exact


def _records(rows):
    """records from rows (n_rec, n_bad, n_cooling, stamp_sum, stamp_min, stamp_max, (q0, q1, q2, q3))"""
    out = {k: np.array([r[i] for r in rows], dtype=np.int64) for i, k in enumerate(SR.FIELDS[:6])}
    out["q"] = np.array([r[6] for r in rows], dtype=np.int64).reshape(len(rows), 4)
    return out


EMPTY = (0, 0, 0, 0, I64MAX, -1, (0, 0, 0, 0))
# plane 0: two good voxels (stamps 20 and 40; one cooling) and a bad one; plane 1: nothing; plane 2: one good voxel, stamp 60
LAYERS = [(2, 1, 1, 60, 20, 40, (40, -12, -3, 48000)), EMPTY, (1, 0, 1, 60, 60, 60, (8, 24, -6, 24008))]
# the same voxels by grain: grain 1 holds the voxels stamped 20 and 60, grain 2 is substrate, grain 3 the one stamped 40 and the bad one
GRAINS = [(2, 0, 2, 80, 20, 60, (24, 4, -5, 48008)), EMPTY, (1, 1, 0, 40, 40, 40, (24, 8, -4, 24000))]
CLUSTERS = {"size": np.array([5, 1, 7]), "bbox": np.array([[0, 0, 0, 2, 0, 1], [1, 1, 1, 1, 1, 1], [0, 1, 0, 1, 2, 2]])}


def _lists(table):
    return {k: [x.item() for x in v] for k, v in table.items()}


def test_columns_planes_and_grains_by_hand(tmp_path):
    import metrics
    assert metrics.SOLID_COLUMNS == ("SolidVoxels", "Remelted", "G_solid", "Gi_solid", "Cool_solid", "T_solid", "V_solid",
                                     "G_over_V_solid")
    m = metrics.solid_metrics(dict(layers=_records(LAYERS), grains=_records(GRAINS)), SCALES, remelted=7, step=60, clusters=CLUSTERS)
    # three good voxels and a bad one; sums over the planes q = (48, 12, -9, 72008), each over 3 x its scale
    assert [m[c] for c in metrics.SOLID_COLUMNS] == [4, 7, 48 / 12.0, 12 / 6.0, -9 / 1.5, 72008 / 24.0, 3.0, 4.0 / 3.0]
    assert (m["G_solid"], m["Gi_solid"], m["Cool_solid"], m["V_solid"]) == (4.0, 2.0, -6.0, 3.0)      # V = -Cool / Gi > 0 when cooling
    assert isinstance(m["SolidVoxels"], int) and isinstance(m["Remelted"], int)
    assert _lists(m["planes"]) == {
        "Step": [60, 60, 60], "plane": [0, 1, 2], "n_rec": [2, 0, 1], "n_bad": [1, 0, 0], "n_cooling": [1, 0, 1],
        "G": [5.0, 0.0, 2.0], "Gi": [-3.0, 0.0, 12.0], "Cool": [-3.0, 0.0, -12.0], "T": [3000.0, 0.0, 3001.0],
        "stamp_first": [20, -1, 60], "stamp_last": [40, -1, 60], "stamp_mean": [30.0, -1.0, 60.0]}
    assert list(m["planes"]) == ["Step", "plane", "n_rec", "n_bad", "n_cooling", "G", "Gi", "Cool", "T", "stamp_first",
                                 "stamp_last", "stamp_mean"]
    assert _lists(m["grains"]) == {
        "id": [1, 2, 3], "n": [5, 1, 7], "aspect": [3.0, 1.0, 1.5], "n_rec": [2, 0, 1], "n_bad": [0, 0, 1], "n_cooling": [2, 0, 0],
        "G": [3.0, 0.0, 6.0], "Gi": [1.0, 0.0, 4.0], "Cool": [-5.0, 0.0, -8.0], "T": [3000.5, 0.0, 3000.0],
        "stamp_first": [20, -1, 40], "stamp_last": [60, -1, 40], "stamp_mean": [40.0, -1.0, 40.0]}
    # the files: a header and one row per plane / grain, in the tables' column order
    metrics.write_solid_csv(tmp_path / "l.csv", [m["planes"], m["planes"]])
    rows = list(csv.reader(open(tmp_path / "l.csv")))
    assert rows[0] == list(m["planes"]) and len(rows) == 7
    assert rows[1] == ["60", "0", "2", "1", "1", "5.0", "-3.0", "-3.0", "3000.0", "20", "40", "30.0"] and rows[4] == rows[1]
    metrics.write_solid_csv(tmp_path / "g.csv", [m["grains"]])
    rows = list(csv.reader(open(tmp_path / "g.csv")))
    assert rows[0] == list(m["grains"]) and rows[3] == ["3", "7", "1.5", "1", "1", "0", "6.0", "4.0", "-8.0", "3000.0", "40", "40", "40.0"]
    # without a clustering the grains table has no size / aspect; without grain records there is no grains table
    m2 = metrics.solid_metrics(dict(layers=_records(LAYERS), grains=_records(GRAINS)), SCALES)
    assert "n" not in m2["grains"] and "aspect" not in m2["grains"] and m2["grains"]["G"].tolist() == [3.0, 0.0, 6.0]
    assert (m2["Remelted"], m2["planes"]["Step"].tolist()) == (0, [0, 0, 0])
    assert "grains" not in metrics.solid_metrics(dict(layers=_records(LAYERS), grains=None), SCALES)


def test_each_quantity_takes_its_own_scale():
    """four different scales: a swapped index or a product in place of the quotient changes a column"""
    import metrics
    sc = (2.0, 8.0, 0.25, 16.0)
    m = metrics.solid_metrics(dict(layers=_records([(4, 0, 0, 0, 0, 0, (64, 64, 64, 64))]), grains=None), sc)
    assert (m["G_solid"], m["Gi_solid"], m["Cool_solid"], m["T_solid"]) == (8.0, 2.0, 64.0, 1.0)
    assert (m["V_solid"], m["G_over_V_solid"]) == (-32.0, -0.25)
    p = m["planes"]
    assert (p["G"][0], p["Gi"][0], p["Cool"][0], p["T"][0]) == (8.0, 2.0, 64.0, 1.0)


def test_gi_zero_and_empty():
    import metrics
    # the build-direction components cancel: V reads 0.0 and G / V inf, the other means stand
    lay = [(1, 0, 1, 20, 20, 20, (8, 6, -4, 24000)), (1, 0, 1, 40, 40, 40, (8, -6, -4, 24000))]
    m = metrics.solid_metrics(dict(layers=_records(lay), grains=None), SCALES)
    assert [m[c] for c in metrics.SOLID_COLUMNS] == [2, 0, 2.0, 0.0, -8.0, 3000.0, 0.0, float("inf")]
    assert m["planes"]["Gi"].tolist() == [3.0, -3.0]
    # no record at all; bad voxels only
    m = metrics.solid_metrics(dict(layers=_records([EMPTY, EMPTY]), grains=_records([])), SCALES, remelted=3)
    assert [m[c] for c in metrics.SOLID_COLUMNS] == [0, 3, 0.0, 0.0, 0.0, 0.0, 0.0, float("inf")]
    assert len(m["grains"]["id"]) == 0 and m["planes"]["stamp_first"].tolist() == [-1, -1]
    m = metrics.solid_metrics(dict(layers=_records([(0, 5, 0, 0, I64MAX, -1, (0, 0, 0, 0))]), grains=None), SCALES)
    assert [m[c] for c in metrics.SOLID_COLUMNS] == [5, 0, 0.0, 0.0, 0.0, 0.0, 0.0, float("inf")]


def test_default_scales_in_physical_units():
    """A ramp of 2 K per voxel edge along the build direction and a field that falls by 0.5 K per microsecond, through the
    comparator with the driver's inv_dx and dt and the default scales: the means come back as 2 K / VOXEL_SIZE in K/m and
    -5e5 K/s, each within half a quantisation step (1 / (2 * scale)) of the exact value, and V = 0.5 K/us / (2 K / edge)."""
    import constants as K
    import metrics
    from cetkmc import engine
    L, dx, dt = 6, float(K.VOXEL_SIZE), 3e-6
    sc = engine.default_solid_scales()
    assert len(sc) == 4 and all(np.isfinite(s) and s > 0 for s in sc)
    T0 = 3000.0 + 2.0 * np.arange(L, dtype=np.float64).reshape(L, 1, 1) + np.zeros((L, L, L))
    T1 = T0 - 1.5                                   # 0.5 K per microsecond over dt = 3 microseconds
    st = np.zeros((L, L, L), np.int64)
    ref = SR.SolidRef(st, T0)
    st[0, 1, 1] = st[2, 3, 4] = st[5, 5, 0] = 1    # a face on either side (one-sided differences) and the inside
    assert ref.update(st, T1, 20, engine._default_inv_dx(), dt)["n_new"] == 3
    m = metrics.solid_metrics(ref.profile(sc), sc, step=20)
    assert m["SolidVoxels"] == 3 and ref.profile(sc)["layers"]["n_bad"].sum() == 0
    g, c = 2.0 / dx, -0.5 / 1e-6                   # K/m (4e5 at 5 um) and K/s
    t = float(np.mean([T1[0, 1, 1], T1[2, 3, 4], T1[5, 5, 0]]))
    slop = 1.0 + 1e-9
    assert abs(m["Gi_solid"] - g) <= 0.5 / sc[1] * slop and abs(m["G_solid"] - g) <= 0.5 / sc[0] * slop
    assert abs(m["Cool_solid"] - c) <= 0.5 / sc[2] * slop
    assert abs(m["T_solid"] - t) <= 0.5 / sc[3] * slop
    # the quantisation steps themselves are small against the quantities: 2^-24 T_MELT per edge, per microsecond, and in K
    assert 0.5 / sc[1] < 1e-4 * g and 0.5 / sc[2] < 1e-3 * abs(c) and 0.5 / sc[3] < 1e-3
    v = 0.25 * dx / 1e-6                           # (0.5 K/us) / (2 K per edge) = a quarter edge per microsecond = 1.25 m/s
    assert abs(m["V_solid"] - v) <= v * (0.5 / sc[2] / abs(c) + 0.5 / sc[1] / g) * 1.01
    assert abs(m["G_over_V_solid"] - g / v) <= (g / v) * 2.0 * (0.5 / sc[2] / abs(c) + 0.5 / sc[1] / g) * 1.01
    assert m["planes"]["n_rec"].tolist() == [1, 0, 1, 0, 0, 1] and abs(m["planes"]["Gi"][2] - g) <= 0.5 / sc[1] * slop
