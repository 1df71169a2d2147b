"""The comparator of the solidification map (solid_ref.py) on hand-computed cases: it is what the device tests compare with,
so its own reading of the definition (include/cetkmc.h) is pinned here, number by number."""
import numpy as np
import pytest

import solid_ref as SR


def _T2():
    # T[i, j, k] = 100 i + 10 j + k on 2^3
    i, j, k = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    return (100.0 * i + 10.0 * j + k).astype(np.float64)


def test_one_new_voxel_2cubed():
    st0 = np.zeros((2, 2, 2), np.int64)
    st0[0, 0, 0] = 1                                   # substrate
    ref = SR.SolidRef(st0, _T2())
    st1 = st0.copy()
    st1[1, 0, 1] = 2
    T1 = _T2() + 4.0
    info = ref.update(st1, T1, stamp=7, inv_dx=2.0, dt=0.5)
    assert info == dict(n_new=1, n_cleared=0, n_recorded=1)
    assert ref.stamp[1, 0, 1] == 7 and (ref.stamp.reshape(-1) >= 0).sum() == 1
    assert ref.stamp[0, 0, 0] == -1                    # the substrate voxel has no record
    assert ref.T_s[1, 0, 1] == 105.0
    # one-sided at every face of a 2^3 lattice: (T[1] - T[0]) * inv_dx
    assert ref.g[1, 0, 1].tolist() == [200.0, 20.0, 2.0]
    assert ref.cool[1, 0, 1] == 8.0                    # (105 - 101) / 0.5
    assert np.array_equal(ref.snap, st1) and np.array_equal(ref.T_snap, T1)


def test_cleared_species_change_and_resolidify_3cubed():
    L = 3
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    T = (i * i * 8.0 + j * 2.0 + k * k).astype(np.float64)
    st0 = np.zeros((L, L, L), np.int64)
    st0[2, 2, 2] = 3
    ref = SR.SolidRef(st0, T)
    st1 = st0.copy()
    st1[1, 1, 1] = 1
    st1[0, 1, 2] = 2
    assert ref.update(st1, T, 20, 1.0, 2.0) == dict(n_new=2, n_cleared=0, n_recorded=2)
    # the centre voxel: central differences * 0.5
    assert ref.g[1, 1, 1].tolist() == [(32.0 - 0.0) * 0.5, (4.0 - 0.0) * 0.5, (4.0 - 0.0) * 0.5]
    # (0, 1, 2): i one-sided low, j central, k one-sided high
    assert ref.g[0, 1, 2].tolist() == [8.0, 2.0, 3.0]
    assert ref.cool[1, 1, 1] == 0.0 and ref.T_s[0, 1, 2] == 6.0
    st2 = st1.copy()
    st2[1, 1, 1] = 3                                   # a change of species: untouched
    st2[0, 1, 2] = 0                                   # cleared
    st2[2, 2, 2] = 0                                   # the substrate voxel empties: cleared, but there was no record
    before = ref.g[1, 1, 1].copy()
    assert ref.update(st2, T + 1.0, 40, 1.0, 2.0) == dict(n_new=0, n_cleared=2, n_recorded=1)
    assert ref.stamp[1, 1, 1] == 20 and np.array_equal(ref.g[1, 1, 1], before)
    assert ref.stamp[0, 1, 2] == -1 and ref.T_s[0, 1, 2] == 0.0 and not ref.g[0, 1, 2].any() and ref.cool[0, 1, 2] == 0.0
    assert not np.signbit(ref.cool[0, 1, 2]) and not np.signbit(ref.g[0, 1, 2]).any()
    st3 = st2.copy()
    st3[0, 1, 2] = 1                                   # solidifies again: the new stamp, cooling against the last snapshot
    assert ref.update(st3, T - 2.0, 60, 1.0, 0.25) == dict(n_new=1, n_cleared=0, n_recorded=2)
    assert ref.stamp[0, 1, 2] == 60 and ref.cool[0, 1, 2] == -12.0 and ref.T_s[0, 1, 2] == 4.0
    ref.begin(st3, T)                                  # a second begin resets
    assert (ref.stamp == -1).all() and not ref.g.any() and np.array_equal(ref.snap, st3)


def test_L1():
    ref = SR.SolidRef(np.zeros((1, 1, 1), np.int64), np.full((1, 1, 1), 5.0))
    assert ref.update(np.ones((1, 1, 1), np.int64), np.full((1, 1, 1), 3.0), 0, 1e9, 1.0) == dict(n_new=1, n_cleared=0, n_recorded=1)
    assert ref.g[0, 0, 0].tolist() == [0.0, 0.0, 0.0] and ref.cool[0, 0, 0] == -2.0 and ref.stamp[0, 0, 0] == 0
    p = ref.profile((1.0, 1.0, 1.0, 1.0))
    assert p["layers"]["n_rec"].tolist() == [1] and p["layers"]["n_cooling"].tolist() == [1] and p["layers"]["q"].tolist() == [[0, 0, -2, 3]]


def test_non_finite_voxel_neighbour_and_snapshot():
    L = 3
    T0 = np.full((L, L, L), 10.0)
    T0[0, 0, 0] = np.nan                               # in the snapshot
    ref = SR.SolidRef(np.zeros((L, L, L), np.int64), T0)
    T1 = np.full((L, L, L), 12.0)
    T1[1, 1, 1] = np.inf                               # on the voxel
    T1[2, 1, 1] = -np.inf                              # a neighbour of (1, 1, 1)
    st = np.zeros((L, L, L), np.int64)
    for v in ((0, 0, 0), (1, 1, 1), (1, 1, 0), (1, 2, 1)):
        st[v] = 1
    ref.update(st, T1, 3, 1.0, 1.0)
    assert np.isnan(ref.cool[0, 0, 0]) and ref.T_s[0, 0, 0] == 12.0 and not ref.g[0, 0, 0].any()
    assert ref.T_s[1, 1, 1] == np.inf and ref.cool[1, 1, 1] == np.inf and ref.g[1, 1, 1, 0] == -np.inf
    assert ref.g[1, 1, 0, 2] == np.inf                 # (T[1,1,1] - T[1,1,0]) * inv_dx at the k = 0 face
    assert ref.g[1, 2, 1, 1] == -np.inf                # (T[1,2,1] - T[1,1,1]) * inv_dx at the j = L - 1 face
    p = ref.profile((1.0, 1.0, 1.0, 1.0))
    assert p["layers"]["n_bad"].tolist() == [1, 3, 0] and not p["layers"]["n_rec"].any()
    assert (p["layers"]["stamp_min"] == SR.NONE_MIN).all() and (p["layers"]["stamp_max"] == -1).all()
    assert not p["layers"]["q"].any() and not p["layers"]["stamp_sum"].any()
    SR.check_identities(ref, p)


def test_saturation_rounding_and_identities():
    L = 4
    st0 = np.zeros((L, L, L), np.int64)
    T = np.zeros((L, L, L))
    ref = SR.SolidRef(st0, T)
    st = st0.copy()
    st[0, 0, 0] = st[0, 0, 1] = st[1, 0, 0] = st[1, 3, 3] = st[3, 0, 0] = 1
    T1 = T.copy()
    T1[0, 0, 0], T1[0, 0, 1], T1[1, 0, 0], T1[1, 3, 3], T1[3, 0, 0] = 0.5, 1.5, 2.5, -2.5, 2.0 ** 38
    ref.update(st, T1, 9, 0.0, 1.0)                    # inv_dx = 0: every gradient is (+-)0 apart from 2^38 * 0 = 0
    scales = (1.0, 1.0, 1.0, 1.0)
    lab = np.zeros((L, L, L), np.int64)
    lab[0, 0, 0] = lab[1, 0, 0] = 1
    lab[0, 0, 1] = 2
    lab[3, 0, 0] = 3                                   # (1, 3, 3) is recorded with label 0
    p = ref.profile(scales, lab)
    lay, gr = p["layers"], p["grains"]
    # ties go to the even integer: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -2.5 -> -2; |x * q| = 2^38 is not below the limit: bad
    assert lay["q"][:, 3].tolist() == [0 + 2, 2 - 2, 0, 0] and lay["q"][:, 2].tolist() == [2, 0, 0, 0]
    assert lay["n_rec"].tolist() == [2, 2, 0, 0] and lay["n_bad"].tolist() == [0, 0, 0, 1]
    assert gr["n_rec"].tolist() == [2, 1, 0] and gr["n_bad"].tolist() == [0, 0, 1] and gr["q"][:, 3].tolist() == [2, 2, 0]
    assert lay["n_cooling"].tolist() == [0, 1, 0, 0]
    assert lay["stamp_sum"].tolist() == [18, 18, 0, 0] and lay["stamp_min"].tolist() == [9, 9, SR.NONE_MIN, SR.NONE_MIN]
    assert lay["stamp_max"].tolist() == [9, 9, -1, -1] and gr["stamp_min"].tolist() == [9, 9, SR.NONE_MIN]
    SR.check_identities(ref, p, scales, lab)
    assert ref.ties(scales) == 5                       # every recorded voxel here sits on a half-integer or on the limit
    T1[3, 0, 0] = 2.0 ** 38 - 4.0                      # below the limit: good
    ref.begin(st0, T)
    ref.update(st, T1, 9, 0.0, 1.0)
    assert ref.profile(scales)["layers"]["n_rec"].tolist() == [2, 2, 0, 1]
    ref.begin(st0, T)
    ref.update(st, np.round(T1) + 0.25, 9, 0.0, 1.0)
    assert ref.ties(scales) == 0


@pytest.mark.parametrize("L", [5, 9])
def test_identities_on_a_sequence(L):
    seq = SR.sequence(L, 3 + L)
    ref = SR.SolidRef(*seq[0])
    lab = np.random.RandomState(L).randint(0, 4, (L, L, L))
    for u, (st, T) in enumerate(seq[1:]):
        info = ref.update(st, T, 20 * u, 1.0, 2.0 ** -u)
        assert info["n_new"] > 0 and info["n_cleared"] > 0
        assert ref.ties(SR.GRID_SCALES) == 0
        p = ref.profile(SR.GRID_SCALES, lab)
        SR.check_identities(ref, p, SR.GRID_SCALES, lab)
        assert info["n_recorded"] == int(p["layers"]["n_rec"].sum() + p["layers"]["n_bad"].sum())
    sp = SR.special_voxels(L)
    assert len(sp) == 26 and all(ref.stamp[v] == 40 for v in sp)       # solidified, cleared and solidified again
    assert len(np.unique(ref.stamp)) == 4                               # -1 and the three stamps
