"""cetkmc_solid_profile against the NumPy comparator (solid_ref.py): every field of every record ==.

The map comes from uploaded states and temperatures (solid_ref.sequence: three updates with three stamps) on a grid of 1/8 K
with power-of-two scales, so that gi, cool and T_s quantise without a tie and only G, a square root, has to be checked
(SolidRef.ties == 0 is asserted first, every time).  The labels are imported (layer_ref.KINDS; they need not agree with the
state, so recorded voxels with label 0 occur in every case) at sizes on both sides of the kernel's wave, pass and block edges
(64, 256 and 2048 voxels in row-major order), plus the three regimes of the reduction by label: one grain, singletons (far
more labels in a block than its table has slots), and the device clustering behind stepping work."""
import functools

import numpy as np
import pytest

import grain_ref as GR
import layer_ref as LR
import solid_ref as SR
from helpers import FOUR_KIND_PARAMS, batch_calls, oracle_lattice, random_lattice

pytestmark = pytest.mark.gpu

SCALES = SR.GRID_SCALES
STAMPS = (3, 20, 4000000000)
KINDS = ("one", "stripes0", "stripes2", "blocks", "scattered")


@functools.lru_cache(maxsize=None)
def _sequence(L):
    seq = SR.sequence(L, 23 + L)
    for st, T in seq:
        st.setflags(write=False)
        T.setflags(write=False)
    return seq


def _mapped(L, seq=None, scales=SCALES):
    """an engine whose map went through the sequence's updates, and the comparator in the same state"""
    import cetkmc
    seq = _sequence(L) if seq is None else seq
    e = cetkmc.Engine(L)
    z = np.zeros((L, L, L))
    e.upload(seq[0][0], z, z, seq[0][1], np.zeros((L, L, L), np.int64))
    e.solid_begin()
    ref = SR.SolidRef(*seq[0])
    for u, (st, T) in enumerate(seq[1:]):
        e.upload(state=st, T=T)
        assert e.solid_update(STAMPS[u], 2.0 ** -u, 1.0) == ref.update(st, T, STAMPS[u], 1.0, 2.0 ** -u)
    assert ref.ties(scales) == 0
    return e, ref


def _labels(kind, L):
    raw, _ = LR.labelling(kind, L, LR.case_seed(kind, L))
    return LR.from_raw(raw)[0].astype(np.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", GR.SHAPES)
def test_shapes(L, kind):
    lab = _labels(kind, L)
    n = int(lab.max())
    e, ref = _mapped(L)
    try:
        e.import_clusters(lab)
        d2h = e.counters()["bytes_d2h"]
        got = e.solid_profile(SCALES, grains=True, recluster=False)
        copied = e.counters()["bytes_d2h"] - d2h
        again = e.solid_profile(SCALES, grains=True, recluster=False)
        plain = e.solid_profile(SCALES)
    finally:
        e.close()
    want = ref.profile(SCALES, lab)
    SR.check_identities(ref, want, SCALES, lab)
    rec = ref.stamp >= 0
    print(f"L={L} {kind}: recorded {int(rec.sum())} of them unlabelled {int((rec & (lab == 0)).sum())} grains {n} "
          f"without a record {int((want['grains']['n_rec'] + want['grains']['n_bad'] == 0).sum())}")
    assert kind not in ("blocks", "scattered") or L < 6 or (rec & (lab == 0)).any()      # labels 0 on recorded voxels
    assert SR.same_records(got["layers"], want["layers"]) == [] and SR.same_records(got["grains"], want["grains"]) == []
    for a, b in ((again["layers"], got["layers"]), (again["grains"], got["grains"]), (plain["layers"], got["layers"])):
        assert SR.same_records(a, b) == []
    assert plain["grains"] is None and copied == (L + n) * SR.REC


def test_one_grain_129_and_empty_planes():
    """every recorded voxel of 129^3 adds to one grain record; only a slab of planes solidifies, the others' records are empty"""
    L = 129
    T = SR.grid_T(L, 1)
    st0 = np.zeros((L, L, L), np.int64)
    st1 = st0.copy()
    st1[40:47] = 1 + (np.arange(L * L).reshape(L, L) % 3)
    st1[100, ::2, ::3] = 2
    seq = [(st0, T), (st1, SR.grid_T(L, 2)), (st1, SR.grid_T(L, 3)), (st1, SR.grid_T(L, 4))]
    e, ref = _mapped(L, seq)
    lab = np.ones((L, L, L), np.int32)
    try:
        e.import_clusters(lab)
        got = e.solid_profile(SCALES, grains=True, recluster=False)
    finally:
        e.close()
    want = ref.profile(SCALES, lab)
    lay = want["layers"]
    assert int(want["grains"]["n_rec"][0]) == 7 * L * L + 65 * 43 == int(lay["n_rec"].sum())
    empty = np.ones(L, bool)
    empty[40:47] = empty[100] = False
    assert (lay["stamp_min"][empty] == SR.NONE_MIN).all() and (lay["stamp_max"][empty] == -1).all() and not lay["n_rec"][empty].any()
    assert (lay["stamp_min"][~empty] == STAMPS[0]).all()
    assert SR.same_records(got["layers"], lay) == [] and SR.same_records(got["grains"], want["grains"]) == []


def test_singletons_33_and_cap():
    L = 33
    lab, _ = GR.singletons(L)
    n = int(lab.max())
    assert n > 100 * 128
    e, ref = _mapped(L)
    try:
        e.import_clusters(lab)
        got = e.solid_profile(SCALES, grains=True, recluster=False)
        want = ref.profile(SCALES, lab)
        SR.check_identities(ref, want, SCALES, lab)
        g = want["grains"]
        assert (g["n_rec"] + g["n_bad"] <= 1).all() and (g["n_rec"] == 0).any() and (g["n_rec"] == 1).any()
        assert (g["stamp_min"][g["n_rec"] == 0] == SR.NONE_MIN).all() and (g["stamp_max"][g["n_rec"] == 0] == -1).all()
        assert SR.same_records(got["layers"], want["layers"]) == [] and SR.same_records(got["grains"], g) == []
        import cetkmc
        rec = np.zeros(n, cetkmc.engine.SOLID_DTYPE)
        for f in SR.FIELDS:
            rec[f] = got["grains"][f]
        a = cetkmc.engine._solid_args(SCALES)
        lay = np.zeros(L, cetkmc.engine.SOLID_DTYPE)
        for cap in (1, n // 2, n, n + 5):
            k = min(cap, n)
            buf = np.zeros(cap + 1, cetkmc.engine.SOLID_DTYPE)
            buf["n_rec"] = -7
            d2h = e.counters()["bytes_d2h"]
            assert e.lib.cetkmc_solid_profile(e.h, a, lay.ctypes.data, cap, buf.ctypes.data) == 0
            assert e.counters()["bytes_d2h"] - d2h == (L + k) * SR.REC
            assert buf[:k].tobytes() == rec[:k].tobytes() and (buf["n_rec"][k:] == -7).all()
        for cap in (0, -3):                                    # no grain record asked for: the planes alone
            lay[:] = 0
            assert e.lib.cetkmc_solid_profile(e.h, a, lay.ctypes.data, cap, buf.ctypes.data) == 0
            assert np.array_equal(lay["q"], want["layers"]["q"]) and (buf["n_rec"][n:] == -7).all()
    finally:
        e.close()


@pytest.mark.parametrize("L", [9, 33])
def test_bad_and_saturating_voxels(L):
    """non-finite temperatures make bad voxels; a temperature scale under which the upper half of the grid saturates"""
    seq = [(st, T.copy()) for st, T in _sequence(L)]
    rs = np.random.RandomState(L)
    for u, (st, T) in enumerate(seq):
        for q, v in enumerate(rs.randint(0, L, (L ** 3 // 10, 3))):
            T[tuple(v)] = (np.nan, np.inf, -np.inf)[(q + u) % 3]
    scales = SCALES[:3] + (2.0 ** 38 / 3000.46875,)
    lab = _labels("scattered", L)
    e, ref = _mapped(L, seq, scales)
    try:
        e.import_clusters(lab)
        got = e.solid_profile(scales, grains=True, recluster=False)
    finally:
        e.close()
    want = ref.profile(scales, lab)
    x = ref.quantities()
    rec = ref.stamp >= 0
    saturated = rec & np.isfinite(x).all(axis=-1) & ~ref.good(scales)
    assert saturated.any() and (rec & ~np.isfinite(x).all(axis=-1)).any() and ref.good(scales).any()
    assert want["layers"]["n_bad"].sum() > saturated.sum() and want["grains"]["n_bad"].any()
    SR.check_identities(ref, want, scales, lab)
    assert SR.same_records(got["layers"], want["layers"]) == [] and SR.same_records(got["grains"], want["grains"]) == []


def test_device_clustering_behind_stepping(oracle_mod):
    """run_steps, update, cluster and profile, all queued on the handle's stream: the profile of the map the oracle's state
    and T give, under the product's default scales, with the labels the device clustering reports"""
    import cetkmc
    L = 16
    lat = random_lattice(L, 47)
    params = cetkmc.default_params(0.2)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=0.2, params=params)
    o = oracle_lattice(oracle_mod, lat, 0.2, FOUR_KIND_PARAMS)
    scales = cetkmc.engine.default_solid_scales()
    try:
        e.upload(*lat)
        e.solid_begin()
        ref = SR.SolidRef(o.state, o.T)
        for step0, n, u_pick, u_def, u_np in batch_calls((20, 20, 20)):
            kw = dict(rng_mode=1, seed=5, thermal_mode=1)
            e.run_steps(step0, n, 0.05, u_pick, u_def, u_np, want_logs=False, **kw)
            o.run_steps(step0, n, 0.05, u_pick, u_def, u_np, **kw)
            assert e.solid_update(step0 + n, 1e-6, 2.0e5) == ref.update(o.state, o.T, step0 + n, 2.0e5, 1e-6)
        assert ref.ties(scales) == 0
        got = e.solid_profile(grains=True)
        lab = e.clusters(0.5, labels=True)["labels"]
        assert SR.same_map(e.solid_read(), ref.map()) == []
    finally:
        e.close()
    want = ref.profile(scales, lab)
    SR.check_identities(ref, want, scales, lab)
    assert int(want["layers"]["n_rec"].sum()) >= 50 and not want["layers"]["n_bad"].any()
    assert (want["grains"]["n_rec"] > 0).sum() >= 2 and want["layers"]["n_cooling"].sum() + want["layers"]["n_rec"].sum() > 0
    assert SR.same_records(got["layers"], want["layers"]) == [] and SR.same_records(got["grains"], want["grains"]) == []


def test_refusals():
    import cetkmc
    L = 8
    lab = _labels("blocks", L)
    n = int(lab.max())
    a = cetkmc.engine._solid_args(SCALES)
    lay = np.zeros(L, cetkmc.engine.SOLID_DTYPE)
    gr = np.zeros(n + 1, cetkmc.engine.SOLID_DTYPE)

    def refused(e, call, text):
        d2h = e.counters()["bytes_d2h"]
        assert call() != 0
        assert text in e.error(), e.error()
        assert e.counters()["bytes_d2h"] == d2h and not lay["n_rec"].any() and not gr["stamp_min"].any()

    e = cetkmc.Engine(L, n_slabs=2)
    try:
        refused(e, lambda: e.lib.cetkmc_solid_profile(e.h, a, lay.ctypes.data, 0, None), "one slab")
    finally:
        e.close()
    e = cetkmc.Engine(L)
    try:
        refused(e, lambda: e.lib.cetkmc_solid_profile(e.h, a, lay.ctypes.data, 0, None), "needs a map")
    finally:
        e.close()
    e, ref = _mapped(L)
    try:
        refused(e, lambda: e.lib.cetkmc_solid_profile(e.h, a, lay.ctypes.data, n, gr.ctypes.data), "needs a preceding cetkmc_cluster")
        with pytest.raises(RuntimeError, match="preceding cetkmc_cluster"):
            e.solid_profile(SCALES, grains=True, recluster=False)
        want = ref.profile(SCALES, lab)
        assert SR.same_records(e.solid_profile(SCALES)["layers"], want["layers"]) == []    # grains == NULL: no clustering needed
        e.import_clusters(lab)
        refused(e, lambda: e.lib.cetkmc_solid_profile(e.h, None, lay.ctypes.data, n, gr.ctypes.data), "null argument")
        refused(e, lambda: e.lib.cetkmc_solid_profile(e.h, a, None, n, gr.ctypes.data), "null argument")
        refused(e, lambda: e.lib.cetkmc_solid_profile(None, a, lay.ctypes.data, n, gr.ctypes.data), "null")
        refused(e, lambda: e.lib.cetkmc_ensemble_solid_profile(e.h, a, lay.ctypes.data, gr.ctypes.data), "not an ensemble handle")
        for c, bad in ((0, 0.0), (1, -1.0), (2, np.nan), (3, np.inf)):
            b = cetkmc.engine._solid_args(tuple(bad if q == c else 1.0 for q in range(4)))
            refused(e, lambda: e.lib.cetkmc_solid_profile(e.h, b, lay.ctypes.data, n, gr.ctypes.data), f"qscale[{c}]")
        got = e.solid_profile(SCALES, grains=True, recluster=False)                         # the handle is still usable
        assert SR.same_records(got["layers"], want["layers"]) == [] and SR.same_records(got["grains"], want["grains"]) == []
    finally:
        e.close()
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * 2)
    try:
        r0 = ens.replica(0)
        z = np.zeros((L, L, L))
        for r in range(2):
            ens.replica(r).upload(_sequence(L)[0][0], z, z, _sequence(L)[0][1], np.zeros((L, L, L), np.int64))
        lay2 = np.zeros((2, L), cetkmc.engine.SOLID_DTYPE)
        refused(r0, lambda: ens.lib.cetkmc_ensemble_solid_profile(ens.h, a, lay2.ctypes.data, None), "cetkmc_ensemble_solid_begin")
        ens.solid_begin()
        refused(r0, lambda: ens.lib.cetkmc_ensemble_solid_profile(ens.h, a, lay2.ctypes.data, gr.ctypes.data), "needs a preceding cetkmc_ensemble_analyze")
        refused(r0, lambda: ens.lib.cetkmc_solid_profile(ens.h, a, lay.ctypes.data, 0, None), "an ensemble handle goes to")
        refused(r0, lambda: ens.lib.cetkmc_ensemble_solid_profile(ens.replica(1).h, a, lay2.ctypes.data, None), "not an ensemble handle")
        refused(r0, lambda: ens.lib.cetkmc_ensemble_solid_profile(ens.h, a, None, None), "null argument")
        assert ens.lib.cetkmc_solid_profile(ens.replica(1).h, a, lay.ctypes.data, 0, None) == 0      # a replica handle is taken
        assert not lay["n_rec"].any() and (lay["stamp_min"] == SR.NONE_MIN).all()
    finally:
        ens.close()
