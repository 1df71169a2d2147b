"""cetkmc_origin_profile against the comparator (origin_ref.py): every field of every record ==.

The map comes from crafted records (three absorb calls, the middle one with group = n: thousands of voxels share one ordinal,
so birth is decided by code and position), the state is random and the labels are imported (layer_ref.KINDS; they need not
agree with the state, so occupied voxels with label 0 and labelled empty voxels occur) at sizes on both sides of the kernel's
wave, pass and block edges (64, 256 and 2048 voxels in row-major order), plus the three regimes of the reduction by label:
one grain, singletons (far more labels in a block than its table has slots), and the device clustering behind real stepping."""
import functools

import numpy as np
import pytest

import grain_ref as GR
import layer_ref as LR
import origin_ref as OR
from helpers import FOUR_KIND_PARAMS, batch_calls, random_lattice

pytestmark = pytest.mark.gpu

KINDS = ("one", "stripes0", "stripes2", "blocks", "scattered")
FIELDS = tuple(f for f in OR.REC_FIELDS if f != "pad")


def _records(L, n, seed):
    rs = np.random.RandomState(seed)
    ev = np.zeros(n, OR.EVENT)
    ev["type"] = rs.randint(-1, 4, n)
    ev["pos"] = rs.randint(0, L, (n, 3))
    ev["target"] = rs.randint(0, L, (n, 3))
    return ev


@functools.lru_cache(maxsize=None)
def _case(L):
    """(state, calls, words, census, seq) of the map at edge L: the comparator's side, computed once"""
    rs = np.random.RandomState(100 + L)
    state = np.where(rs.random_sample((L,) * 3) < 0.6, rs.randint(1, 5, (L,) * 3), 0).astype(np.int64)
    n = int(min(max(L ** 3, 4), 40000))
    calls = ((_records(L, n, L), 1), (_records(L, n, 2 * L), n), (_records(L, n // 4, 3 * L), 1))
    words, census, seq = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64), 0
    for ev, group in calls:
        seq = OR.absorb(words, census, ev, seq, group, L)
    for a in (state, words, census):
        a.setflags(write=False)
    return state, calls, words, census, seq


def _mapped(L, state=None):
    import cetkmc
    st, calls, words, census, seq = _case(L)
    e = cetkmc.Engine(L)
    z = np.zeros((L,) * 3)
    e.upload(st if state is None else state, z, z, z + 3000.0, np.zeros((L,) * 3, np.int64))
    e.origin_begin()
    for ev, group in calls:
        e.origin_absorb(ev, group)
    assert np.array_equal(e.origin_words(), words) and np.array_equal(e.origin_census(), census) and e.origin_seq() == seq
    return e


def _diff(got, want):
    """the fields in which a profile dict of the engine differs from the comparator's records"""
    return [f for f in FIELDS if not np.array_equal(got[f], want[f])]


def _labels(kind, L):
    raw, _ = LR.labelling(kind, L, LR.case_seed(kind, L))
    return LR.from_raw(raw)[0].astype(np.int32)


@pytest.mark.parametrize("L", GR.SHAPES)
def test_shapes(L):
    state, _, words, _, _ = _case(L)
    e = _mapped(L)
    try:
        plain = e.origin_profile()                             # grains=None needs no clustering
        with pytest.raises(RuntimeError, match="needs a preceding cetkmc_cluster"):
            e.origin_profile(grains=True, recluster=False)
        lay_want, _ = OR.profile(words, state)
        assert plain["grains"] is None and _diff(plain["layers"], lay_want) == []
        for kind in KINDS:
            lab = _labels(kind, L)
            n = int(lab.max())
            e.import_clusters(lab)
            d2h = e.counters()["bytes_d2h"]
            got = e.origin_profile(grains=True, recluster=False)
            copied = e.counters()["bytes_d2h"] - d2h
            again = e.origin_profile(grains=True, recluster=False)
            lay, gr = OR.profile(words, state, lab, n)
            tag = f"L={L} {kind}"
            assert _diff(got["layers"], lay) == [] and _diff(got["grains"], gr) == [], tag
            assert all(got[p][f].tobytes() == again[p][f].tobytes() for p in ("layers", "grains") for f in FIELDS), tag
            assert copied == (L + n) * OR.REC.itemsize, tag
            assert int(gr["n_left"].sum()) == 0 and int(gr["n_occ"].sum()) == int((lab > 0).sum())
            if L >= 7 and kind in ("blocks", "scattered"):     # the cases are not vacuous
                assert ((state != 0) & (lab == 0)).any() and ((state == 0) & (lab != 0)).any(), tag
        o, code = OR.decode(words)
        if L >= 7:
            assert lay_want["n_left"].sum() > 0 and lay_want["n_unrec"].sum() > 0 and (lay_want["n_by"].sum(axis=0) > 0).all()
            tied = o == np.bincount(o[o >= 0]).argmax()
            assert tied.sum() > 50                             # the ordinal of the group = n call
    finally:
        e.close()


def test_one_grain_129_and_empty_planes():
    """every voxel of 129^3 adds to one grain record; only a slab of planes is occupied, the other planes count the voxels
    that were left and nothing else"""
    L = 129
    _, _, words, _, _ = _case(L)
    state = np.zeros((L,) * 3, np.int64)
    state[40:47] = 1 + (np.arange(L * L).reshape(L, L) % 3)
    state[100, ::2, ::3] = 2
    lab = np.ones((L,) * 3, np.int32)
    e = _mapped(L, state)
    try:
        e.import_clusters(lab)
        got = e.origin_profile(grains=True, recluster=False)
    finally:
        e.close()
    lay, gr = OR.profile(words, state, lab, 1)
    empty = np.ones(L, bool)
    empty[40:47] = empty[100] = False
    assert not lay["n_occ"][empty].any() and (lay["ord_min"][empty] == OR.INT64_MAX).all() and (lay["ord_max"][empty] == -1).all()
    assert int(lay["n_occ"].sum()) == 7 * L * L + 65 * 43 and int(gr["n_occ"][0]) == L ** 3
    assert lay["n_left"].sum() > 0 and lay["n_by"].sum() > 0
    assert _diff(got["layers"], lay) == [] and _diff(got["grains"], gr) == []


def test_singletons_33_and_cap():
    import cetkmc
    L = 33
    state, _, words, _, _ = _case(L)
    lab, _ = GR.singletons(L)
    n = int(lab.max())
    assert n > 100 * 128
    e = _mapped(L)
    try:
        e.import_clusters(lab)
        got = e.origin_profile(grains=True, recluster=False)
        lay, gr = OR.profile(words, state, lab, n)
        assert (gr["n_occ"] == 1).all() and (gr["n_unrec"] == 1).any() and (gr["n_by"].sum(axis=1) == 1).any()
        assert (gr["birth"][gr["n_unrec"] == 1] == OR.INT64_MAX).all()
        assert _diff(got["layers"], lay) == [] and _diff(got["grains"], gr) == []
        DT = cetkmc.engine.ORIGIN_DTYPE
        layb = np.zeros(L, DT)
        for cap in (1, n // 2, n, n + 5):
            k = min(cap, n)
            buf = np.zeros(cap + 1, DT)
            buf["n_occ"] = -7
            d2h = e.counters()["bytes_d2h"]
            assert e.lib.cetkmc_origin_profile(e.h, layb.ctypes.data, cap, buf.ctypes.data) == 0
            assert e.counters()["bytes_d2h"] - d2h == (L + k) * 96
            assert buf[:k].tobytes() == gr[:k].tobytes() and (buf["n_occ"][k:] == -7).all()
            assert layb.tobytes() == lay.tobytes()
        for cap in (0, -3):                                    # no grain record asked for: the planes alone
            layb[:] = 0
            assert e.lib.cetkmc_origin_profile(e.h, layb.ctypes.data, cap, buf.ctypes.data) == 0
            assert layb.tobytes() == lay.tobytes() and (buf["n_occ"][n:] == -7).all()
    finally:
        e.close()


def test_device_clustering_behind_stepping():
    """the profile by the device's own clustering after real stepping with a map: records from the words, the state and the
    labels the engine returns"""
    import cetkmc
    L = 16
    params = cetkmc.default_params(0.2)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=0.2, params=params)
    try:
        e.upload(*random_lattice(L, 12))
        e.origin_begin()
        for step0, n, u_pick, u_def, u_np in batch_calls((40, 40)):
            r = e.run_steps(step0, n, 0.05, u_pick, u_def, u_np, rng_mode=1, seed=5, thermal_mode=1)
            assert (r["done"], r["status"]) == (n, 0)
        assert e.origin_seq() == 80
        got = e.origin_profile(grains=True, threshold=0.5)
        again = e.origin_profile(grains=True, recluster=False)
        cl = e.clusters(0.5, labels=True)
        words, state = e.origin_words(), e.download()["state"]
        lay, gr = OR.profile(words, state, cl["labels"], len(cl["size"]))
        assert _diff(got["layers"], lay) == [] and _diff(got["grains"], gr) == []
        assert all(got[p][f].tobytes() == again[p][f].tobytes() for p in ("layers", "grains") for f in FIELDS)
        assert np.array_equal(gr["n_occ"], cl["size"]) and int(lay["n_by"].sum()) > 20 and int(gr["n_left"].sum()) == 0
        assert int(lay["n_occ"].sum()) == int((state != 0).sum())
    finally:
        e.close()
