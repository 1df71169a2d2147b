"""metrics.origin_metrics and metrics.write_origin_csv pinned without a GPU on a hand-written profile and census, number by
number: the fourteen columns, the planes table and the grains table (a nucleation-born grain, a deposition-born one, a
substrate grain, a grain without a voxel), and the empty case."""
import csv

import numpy as np

I64MAX = np.iinfo(np.int64).max


def _records(rows):
    """records from rows (n_occ, (dep, nuc, att, hop), n_unrec, n_left, ord_sum, ord_min, ord_max, birth)"""
    names = ("n_occ", None, "n_unrec", "n_left", "ord_sum", "ord_min", "ord_max", "birth")
    out = {k: np.array([r[i] for r in rows], dtype=np.int64) for i, k in enumerate(names) if k}
    out["n_by"] = np.array([r[1] for r in rows], dtype=np.int64).reshape(len(rows), 4)
    return out


def _birth(o, code, lin):
    return (o << 27) | (code << 24) | lin


EMPTY = (0, (0, 0, 0, 0), 0, 0, 0, I64MAX, -1, I64MAX)
# plane 0: 5 occupied -- 1 dep (ordinal 4), 2 nuc (6, 9), 2 substrate; plane 1: nothing; plane 2: 4 occupied -- 1 nuc (12), 2 att (13, 20),
# 1 hop (30), and one voxel a diffusion left
LAYERS = [(5, (1, 2, 0, 0), 2, 0, 19, 4, 9, _birth(4, 1, 3)), EMPTY, (4, (0, 1, 2, 1), 0, 1, 75, 12, 30, _birth(12, 2, 40))]
# grain 1: the substrate with the deposited voxel on it; grain 2: born by the nucleation 6, grew by the attachments 13 and 20;
# grain 3: the single nucleated voxel 9; grain 4: nucleated voxel 12 with the hopped atom 30; grain 5 has no voxel
GRAINS = [(3, (1, 0, 0, 0), 2, 0, 4, 4, 4, _birth(4, 1, 3)),
          (3, (0, 1, 2, 0), 0, 0, 39, 6, 20, _birth(6, 2, 5)),
          (1, (0, 1, 0, 0), 0, 0, 9, 9, 9, _birth(9, 2, 7)),
          (2, (0, 1, 0, 1), 0, 0, 42, 12, 30, _birth(12, 2, 40)),
          EMPTY]
CENSUS = np.array([[1, 0, 2, 0, 0], [0, 3, 1, 0, 0], [0, 0, 1, 2, 3]], np.int64)      # a nucleation in plane 1 was overwritten


def _lists(table):
    return {k: [x.item() for x in v] for k, v in table.items()}


def test_columns_planes_and_grains_by_hand(tmp_path):
    import metrics
    assert metrics.ORIGIN_COLUMNS == ("Origin_dep", "Origin_nuc", "Origin_att", "Origin_hop", "Origin_unrecorded",
                                      "Nucleated_voxel_frac", "Grains_born_nuc", "Grains_born_dep", "Grains_born_att",
                                      "Grains_born_hop", "Grains_substrate", "Nucleated_grain_volume_frac", "Nuc_events",
                                      "Nuc_events_mean_i")
    m = metrics.origin_metrics(dict(layers=_records(LAYERS), grains=_records(GRAINS)), CENSUS, step=60)
    # fills: 1 dep, 3 nuc, 2 att, 1 hop = 7; grains 2, 3, 4 are nucleation-born with 3 + 1 + 2 = 6 of the 9 labelled voxels;
    # grain 1 is substrate (n_unrec 2); 4 nucleation events at planes 0, 0, 1, 2
    assert [m[c] for c in metrics.ORIGIN_COLUMNS] == [1, 3, 2, 1, 2, 3 / 7.0, 3, 0, 0, 0, 1, 6 / 9.0, 4, 3 / 4.0]
    assert _lists(m["planes"]) == {
        "Step": [60, 60, 60], "plane": [0, 1, 2], "n_occ": [5, 0, 4], "n_dep": [1, 0, 0], "n_nuc": [2, 0, 1], "n_att": [0, 0, 2],
        "n_hop": [0, 0, 1], "n_unrec": [2, 0, 0], "n_left": [0, 0, 1], "ord_first": [4, -1, 12], "ord_last": [9, -1, 30],
        "ord_mean": [19 / 3.0, -1.0, 75 / 4.0], "birth_code": [1, 0, 2], "birth_voxel": [3, -1, 40],
        "ev_dep": [1, 0, 0], "ev_diff_out": [0, 3, 0], "ev_nuc": [2, 1, 1], "ev_att": [0, 0, 2], "ev_diff_in": [0, 0, 3]}
    assert _lists(m["grains"]) == {
        "id": [1, 2, 3, 4, 5], "n_occ": [3, 3, 1, 2, 0], "n_dep": [1, 0, 0, 0, 0], "n_nuc": [0, 1, 1, 1, 0], "n_att": [0, 2, 0, 0, 0],
        "n_hop": [0, 0, 0, 1, 0], "n_unrec": [2, 0, 0, 0, 0], "n_left": [0, 0, 0, 0, 0], "ord_first": [4, 6, 9, 12, -1],
        "ord_last": [4, 20, 9, 30, -1], "ord_mean": [4.0, 13.0, 9.0, 21.0, -1.0], "birth_code": [1, 2, 2, 2, 0],
        "birth_voxel": [3, 5, 7, 40, -1]}
    path = tmp_path / "origin_layers.csv"
    metrics.write_origin_csv(str(path), [m["planes"], m["planes"]])
    rows = list(csv.reader(open(path)))
    assert rows[0] == list(m["planes"]) and len(rows) == 7
    assert rows[1][:6] == ["60", "0", "5", "1", "2", "0"] and rows[3] == rows[6]
    gpath = tmp_path / "origin_grains.csv"
    metrics.write_origin_csv(str(gpath), [m["grains"]])
    rows = list(csv.reader(open(gpath)))
    assert rows[0][0] == "id" and len(rows) == 6 and rows[2][:2] == ["2", "3"]


def test_born_by_other_codes_and_no_grains():
    import metrics
    grains = [(2, (1, 0, 1, 0), 0, 0, 5, 2, 3, _birth(2, 1, 0)),        # deposition first, then an attachment
              (1, (0, 0, 1, 0), 0, 0, 8, 8, 8, _birth(8, 3, 9)),        # an attachment alone (its grain was split off)
              (1, (0, 0, 0, 1), 0, 0, 9, 9, 9, _birth(9, 4, 11))]       # a hopped atom alone
    m = metrics.origin_metrics(dict(layers=_records([EMPTY]), grains=_records(grains)), np.zeros((1, 5), np.int64))
    assert [m[c] for c in metrics.ORIGIN_COLUMNS] == [0, 0, 0, 0, 0, 0.0, 0, 1, 1, 1, 0, 0.0, 0, 0.0]
    m = metrics.origin_metrics(dict(layers=_records([EMPTY, EMPTY]), grains=None), np.zeros((2, 5), np.int64))
    assert [m[c] for c in metrics.ORIGIN_COLUMNS] == [0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0, 0.0, 0, 0.0]
    assert "grains" not in m and _lists(m["planes"])["ord_last"] == [-1, -1]
