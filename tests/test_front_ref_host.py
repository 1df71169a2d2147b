"""The front-diagnostics comparator (front_ref.py) pinned on hand-computed 2^3 and 3^3 lattices, and the host side of the
feature (struct mirror, metrics.front_metrics, V_front) -- no GPU."""
import math

import numpy as np

from front_ref import front_ref, front_ref_stats, gradient_component

INV_DX = 2.0        # half_inv_dx = 1.0: the hand values below stay integers


def _T2():
    i, j, k = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    return (100.0 * i + 10.0 * j + 1.0 * k) + 7.0


def _T3():
    i, j, k = np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    return 100.0 * i * i + 10.0 * j * j + 1.0 * k * k + 5.0


# 3^3, T = 100 i^2 + 10 j^2 + k^2 + 5, inv_dx = 2:  x = 0: (T[1] - T[0]) * 2, x = 1: (T[2] - T[0]) * 1, x = 2: (T[2] - T[1]) * 2
GI3, GJ3, GK3 = (200.0, 400.0, 600.0), (20.0, 40.0, 60.0), (2.0, 4.0, 6.0)


def test_gradient_one_sided_at_both_ends_of_each_axis():
    T = _T3()
    for axis, tab in enumerate((GI3, GJ3, GK3)):
        g = np.moveaxis(gradient_component(T, axis, INV_DX), axis, 0)
        for x in range(3):
            assert np.all(g[x] == tab[x]), (axis, x)
    T = _T2()       # L = 2: no interior, both ends one-sided and equal
    for axis, v in enumerate((200.0, 20.0, 2.0)):
        assert np.all(gradient_component(T, axis, INV_DX) == v)
    assert np.all(gradient_component(np.full((1, 1, 1), 3.0), 0, INV_DX) == 0.0)


def test_2cube_all_corners_front():
    """(0,0,0) and (1,1,1) empty: each of the other six voxels touches one of them."""
    state = np.array([[[0, 1], [2, 3]], [[4, 1], [2, 0]]])
    T = _T2()
    ref = front_ref(state, T, 1e9, INV_DX)
    assert ref["front"].sum() == 6 and not ref["front"][0, 0, 0] and not ref["front"][1, 1, 1]
    assert ref["skipped"].sum() == 0 and ref["melt"].sum() == 0
    G = math.sqrt(200.0 * 200.0 + 20.0 * 20.0 + 2.0 * 2.0)
    assert np.all(ref["G"] == G) and np.all(ref["gi"] == 200.0)
    s = front_ref_stats(ref, T)
    assert s["n_front"] == 6 and list(s["pos_sum"]) == [3, 3, 3]
    assert s["G_min"] == s["G_max"] == G and s["G_sum"] == math.fsum([G] * 6) and s["Gi_sum"] == 1200.0
    assert s["T_sum"] == float(T.sum() - T[0, 0, 0] - T[1, 1, 1])
    assert list(s["melt_bbox"]) == [2, 2, 2, -1, -1, -1] and s["n_melt"] == 0


def test_out_of_lattice_neighbours_do_not_count():
    for L in (1, 2, 3):
        ref = front_ref(np.full((L, L, L), 2), np.full((L, L, L), 1.0), 1e9, INV_DX)
        assert ref["front"].sum() == 0 and ref["skipped"].sum() == 0
        s = front_ref_stats(ref, np.full((L, L, L), 1.0))
        assert s["n_front"] == 0 and s["G_min"] == 0.0 and s["G_max"] == 0.0 and s["G_sum"] == 0.0
    ref = front_ref(np.zeros((3, 3, 3), int), _T3(), 1e9, INV_DX)       # nothing occupied
    assert ref["front"].sum() == 0
    assert front_ref(np.zeros((1, 1, 1), int), np.ones((1, 1, 1)), 0.5, INV_DX)["melt"].sum() == 1


def test_3cube_faces_and_corners_front_centre_not():
    """The 12 edge midpoints empty: the 8 corners and the 6 face centres are front voxels, the centre (whose six neighbours
    are the occupied face centres) is not."""
    state = np.ones((3, 3, 3), int)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                if [i, j, k].count(1) == 1:           # an edge midpoint
                    state[i, j, k] = 0
                elif (i, j, k) != (1, 1, 1):
                    state[i, j, k] = 1 + (i + j + k) % 4
    T = _T3()
    assert (state == 0).sum() == 12
    ref = front_ref(state, T, 1e9, INV_DX)
    want = []
    for i in range(3):
        for j in range(3):
            for k in range(3):
                n1 = [i, j, k].count(1)
                if n1 in (0, 2):
                    want.append((i, j, k))
    assert sorted(map(tuple, np.argwhere(ref["front"]))) == sorted(want) and len(want) == 14
    assert not ref["front"][1, 1, 1]
    for (i, j, k) in want:
        assert ref["gi"][i, j, k] == GI3[i] and ref["gj"][i, j, k] == GJ3[j] and ref["gk"][i, j, k] == GK3[k]
        assert ref["G"][i, j, k] == math.sqrt(GI3[i] * GI3[i] + GJ3[j] * GJ3[j] + GK3[k] * GK3[k])
    s = front_ref_stats(ref, T)
    # corners: 4 with i = 0, 4 with i = 2 -> 8; face centres: 0 + 2 + 1 + 1 + 1 + 1 = 6
    assert s["n_front"] == 14 and list(s["pos_sum"]) == [14, 14, 14]
    assert s["Gi_sum"] == 4 * 200.0 + 4 * 600.0 + (200.0 + 600.0 + 4 * 400.0)
    assert s["G_min"] == math.sqrt(200.0 ** 2 + 20.0 ** 2 + 2.0 ** 2)      # corner (0,0,0)
    assert s["G_max"] == math.sqrt(600.0 ** 2 + 60.0 ** 2 + 6.0 ** 2)      # corner (2,2,2)


def test_3cube_interior_voxel_central_differences():
    state = np.zeros((3, 3, 3), int)
    state[1, 1, 1] = 3
    T = _T3()
    ref = front_ref(state, T, 1e9, INV_DX)
    assert list(map(tuple, np.argwhere(ref["front"]))) == [(1, 1, 1)]
    assert ref["gi"][1, 1, 1] == 400.0 and ref["gj"][1, 1, 1] == 40.0 and ref["gk"][1, 1, 1] == 4.0
    s = front_ref_stats(ref, T)
    assert s["G_sum"] == s["G_min"] == s["G_max"] == math.sqrt(400.0 * 400.0 + 40.0 * 40.0 + 4.0 * 4.0)
    assert s["T_sum"] == 100.0 + 10.0 + 1.0 + 5.0 and list(s["pos_sum"]) == [1, 1, 1]


def test_non_finite_skipped_and_melt():
    state = np.zeros((3, 3, 3), int)
    state[1, 1, 1] = 1
    state[0, 0, 0] = 2
    T = _T3()
    T[0, 1, 1] = np.nan          # neighbour of the front voxel (1,1,1): its gi is NaN
    T[0, 0, 0] = np.inf          # a front voxel's own T; also a melt voxel
    T[2, 2, 2] = -np.inf         # no front voxel, not melt
    T[2, 0, 1] = 700.0           # melt (>= 700)
    ref = front_ref(state, T, 700.0, INV_DX)
    assert ref["front"].sum() == 0 and ref["skipped"].sum() == 2
    s = front_ref_stats(ref, T)
    assert s["n_skipped"] == 2 and s["n_front"] == 0 and s["G_sum"] == 0.0
    # melt: +inf at (0,0,0), 700 at (2,0,1), and T3 >= 700 nowhere else (max finite 100*4 + 10*4 + 4 + 5 = 449)
    assert s["n_melt"] == 2 and list(s["melt_bbox"]) == [0, 0, 0, 2, 0, 1]


def test_struct_mirror_and_dtype():
    import ctypes as C

    from cetkmc import _lib
    assert C.sizeof(_lib.FrontStats) == 112
    assert "cetkmc_front_stats" in _lib.PROTOTYPES and "cetkmc_ensemble_front_stats" in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.cetkmc_struct_size(b"front_stats") == 112
    import cetkmc.engine as eng
    assert eng.FRONT_DTYPE.itemsize == 112
    for name, _ in _lib.FrontStats._fields_:
        assert eng.FRONT_DTYPE.fields[name][1] == getattr(_lib.FrontStats, name).offset, name


def test_front_metrics_and_velocity():
    import metrics
    from constants import T_MELT, VOXEL_SIZE
    st = dict(n_front=4, n_skipped=1, pos_sum=np.array([10, 4, 6]), G_sum=8.0e6, G_min=1.0e6, G_max=3.0e6, Gi_sum=-4.0e6,
              T_sum=12000.0, n_melt=5, melt_bbox=np.array([7, 0, 2, 9, 3, 2], np.int32))
    m = metrics.front_metrics(st, 10, VOXEL_SIZE)
    assert m == {"G_front": 2.0e6, "G_front_max": 3.0e6, "Gi_front": -1.0e6, "T_front": 3000.0,
                 "Undercooling_front": float(T_MELT) - 3000.0, "Front_i": 2.5, "FrontVoxels": 4, "MeltVoxels": 5,
                 "MeltDepth": 3, "MeltLength": 4, "MeltWidth": 1}
    assert tuple(m) == metrics.FRONT_COLUMNS
    empty = dict(n_front=0, n_skipped=0, pos_sum=np.zeros(3, np.int64), G_sum=0.0, G_min=0.0, G_max=0.0, Gi_sum=0.0, T_sum=0.0,
                 n_melt=0, melt_bbox=np.array([10, 10, 10, -1, -1, -1], np.int32))
    e = metrics.front_metrics(empty, 10, VOXEL_SIZE)
    assert all(e[k] == 0 for k in metrics.FRONT_COLUMNS)
    a, b = dict(m, Time=1.0e-9), dict(m, Time=3.0e-9, Front_i=4.5)
    assert metrics.front_velocity(a, None) == 0.0
    assert metrics.front_velocity(b, a) == (4.5 - 2.5) * VOXEL_SIZE / (3.0e-9 - 1.0e-9)
    assert metrics.front_velocity(dict(b, Time=1.0e-9), a) == 0.0
    assert metrics.front_velocity(b, dict(e, Time=0.0)) == 0.0 and metrics.front_velocity(dict(e, Time=5.0), a) == 0.0
