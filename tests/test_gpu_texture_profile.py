"""cetkmc_texture_profile against the NumPy comparator (texture_ref.py): every counter equal.  The counters bin floating-point
values, so every case first asserts -- on the comparator alone -- that none of its values lies within 1e-12 of an edge
(texture_ref.ambiguous: the device's sincos and NumPy's differ by a few ulp, < 3e-15 in a dot product), and then compares
with ==, also against the two identities with cetkmc_layer_profile on the same handle.

Imported labellings (a random partition, slabs along each axis, a sheared checkerboard) put same-label and other-label
predecessors across every tile, rim and plane-group edge of the kernel (8 rows, 32 columns, 16 planes;
texture_ref.check_not_vacuous, pinned on the host in test_texture_ref_host.py); shapes from both sides of every such edge,
n_bins 1, 2, 16, 64, non-finite orientations, a caller's axis, the device clustering behind real stepping, repeated calls,
NULL outputs and every refusal."""
import ctypes as C

import numpy as np
import pytest

import layer_ref as LR
import texture_ref as TR

pytestmark = pytest.mark.gpu

SHAPES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65)
BINS = (1, 2, 16, 64)


def _upload(e, L, labels, theta, phi):
    e.upload(np.where(np.asarray(labels) != 0, 1, 0).astype(np.int64), theta, phi, np.full((L, L, L), 3000.0),
             np.zeros((L, L, L), np.int64))


def _bytes(p):
    return b"".join(np.ascontiguousarray(p[k]).tobytes() for k in TR.FIELDS)


def _want(lab, theta, phi, nb, axis=(1.0, 0.0, 0.0), values=None):
    """the comparator's profile at the default edges of n_bins = nb, after asserting that no value is near an edge"""
    ge, pe = TR.edges_cos(nb, 180.0), TR.edges_cos(nb, 90.0)
    if values is None:
        values = (TR.face_values(lab, theta, phi), TR.pole_values(lab, theta, phi, axis))
    assert TR.n_ambiguous(values, ge, pe) == 0
    return TR.texture_ref(lab, theta, phi, ge, pe, axis, values=values)


def _identities(got, layer):
    assert np.array_equal(got["gb_hist"].sum(axis=2) + got["bad"][:, :3], layer["cut"])
    assert np.array_equal(got["pole_hist"].sum(axis=1) + got["bad"][:, 3], layer["n_occ"])


@pytest.mark.parametrize("L", SHAPES)
def test_shapes(L):
    import cetkmc
    theta, phi = TR.random_angles(L)
    e = cetkmc.Engine(L)
    try:
        for kind in TR.KINDS:
            lab = TR.labelling(kind, L)
            TR.check_not_vacuous(kind, L, lab)
            values = (TR.face_values(lab, theta, phi), TR.pole_values(lab, theta, phi, (1.0, 0.0, 0.0)))
            _upload(e, L, lab, theta, phi)
            e.import_clusters(lab)
            layer = e.layer_profile(recluster=False)
            for nb in BINS:
                want = _want(lab, theta, phi, nb, values=values)
                d2h = e.counters()["bytes_d2h"]
                got = e.texture_profile(n_bins=nb, recluster=False)
                assert e.counters()["bytes_d2h"] - d2h == L * (4 * nb + 4) * 8
                print(f"L={L} {kind} n_bins={nb}: faces {got['gb_hist'].sum(axis=(0, 2)).tolist()} voxels {int(got['pole_hist'].sum())}")
                assert TR.same(got, want) == [], (kind, nb)
                assert not got["bad"].any()
                _identities(got, layer)
                assert _bytes(e.texture_profile(n_bins=nb, recluster=False)) == _bytes(got), (kind, nb)
            if L >= 8 and kind in ("scattered", "checker"):       # guards against a vacuous pass
                assert all(got["gb_hist"][:, a].sum() > 0 for a in range(3)) and np.count_nonzero(got["gb_hist"]) > 64
    finally:
        e.close()


def test_L129():
    """past 128: five column tiles, a ragged last row tile, nine plane groups"""
    import cetkmc
    L, nb = 129, 64
    theta, phi = TR.random_angles(L)
    lab = TR.labelling("scattered", L)
    want = _want(lab, theta, phi, nb)
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, lab, theta, phi)
        e.import_clusters(lab)
        got = e.texture_profile(n_bins=nb, recluster=False)
        layer = e.layer_profile(recluster=False)
    finally:
        e.close()
    assert TR.same(got, want) == []
    _identities(got, layer)


def test_nonfinite_orientations_and_axis():
    """NaN / inf angles go to bad and to no bin; a caller's axis, not normalised (|c| up to 3: above every edge, bin 0)."""
    import cetkmc
    L, nb, axis = 17, 16, (1.0, 2.0, -2.0)
    theta, phi = TR.random_angles(L, s=1)
    rs = np.random.RandomState(3)
    at = rs.random_sample((L, L, L))
    theta[at < 0.02] = np.nan
    phi[(at >= 0.02) & (at < 0.04)] = np.inf
    theta[(at >= 0.04) & (at < 0.05)] = -np.inf
    lab = TR.labelling("checker", L)
    want = _want(lab, theta, phi, nb, axis)
    plain = _want(lab, theta, phi, nb)
    assert (want["bad"].sum(axis=0) > 0).all() and want["pole_hist"][:, 0].sum() > plain["pole_hist"][:, 0].sum()
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, lab, theta, phi)
        e.import_clusters(lab)
        got = e.texture_profile(n_bins=nb, axis=axis, recluster=False)
        got_plain = e.texture_profile(n_bins=nb, recluster=False)
        layer = e.layer_profile(recluster=False)
        # a caller's edges: unequal steps
        gd, pd = np.array([1.0, 7.0, 33.0, 90.5, 179.0]), np.array([0.5, 20.0, 45.0, 60.0, 89.0])
        ge, pe = np.cos(np.deg2rad(gd)), np.cos(np.deg2rad(pd))
        values = (TR.face_values(lab, theta, phi), TR.pole_values(lab, theta, phi, axis))
        assert TR.n_ambiguous(values, ge, pe) == 0
        own = e.texture_profile(n_bins=6, gb_edges_deg=gd, pole_edges_deg=pd, axis=axis, recluster=False)
    finally:
        e.close()
    assert TR.same(got, want) == [] and TR.same(got_plain, plain) == []
    assert TR.same(own, TR.texture_ref(lab, theta, phi, ge, pe, axis, values=values)) == []
    assert np.array_equal(own["gb_edges_deg"], gd) and np.array_equal(own["pole_edges_deg"], pd)
    _identities(got, layer)
    _identities(own, layer)


@pytest.mark.parametrize("L", (16, 33))
def test_after_stepping(L):
    """run_steps, then cluster, then the profile, all queued on the handle's stream directly behind the stepping work: the
    profile of the labels and orientations a download shows."""
    import cetkmc
    import constants as K
    state, theta, phi = LR.random_blocks(L, 100 + L)           # filled boxes of random orientation, 30 % empty
    ramp = float(K.T_SUB) + (float(K.T_MELT) - float(K.T_SUB)) * (np.arange(L) / (L - 1))
    T = np.ascontiguousarray(np.broadcast_to(ramp[:, None, None], (L, L, L)))
    e = cetkmc.Engine(L, impurity_c=0.1)
    try:
        e.upload(state, theta, phi, T, np.zeros((L, L, L), np.int64))
        before = e.texture_profile()
        r = e.run_steps(0, 60, 0.0, None, None, None, rng_mode=2, seed=5, thermal_mode=1)
        assert r["done"] == 60 and r["status"] == 0
        got = e.texture_profile()                               # clusters, then profiles, behind the steps
        again = e.texture_profile(recluster=False)
        layer = e.layer_profile(recluster=False)
        cl = e.clusters(0.5, labels=True)
        now = e.download(T=False)
    finally:
        e.close()
    assert not np.array_equal(now["state"], state)
    assert np.array_equal(cl["labels"] != 0, now["state"] != 0)
    want = _want(cl["labels"], now["theta"], now["phi"], 36)
    assert TR.same(got, want) == [] and _bytes(got) == _bytes(again) and _bytes(got) != _bytes(before)
    _identities(got, layer)
    assert got["gb_hist"].sum() > 0 and not got["bad"].any()


def _args(nb, ge, pe, axis=(1.0, 0.0, 0.0)):
    from cetkmc import _lib
    a = _lib.TextureArgs()
    a.n_bins = nb
    keep = [None if x is None else np.ascontiguousarray(x, np.float64) for x in (ge, pe)]
    a.gb_edges = None if keep[0] is None else keep[0].ctypes.data_as(C.POINTER(C.c_double))
    a.pole_edges = None if keep[1] is None else keep[1].ctypes.data_as(C.POINTER(C.c_double))
    a.axis[:] = axis
    return a, keep


def test_null_outputs():
    """any of the three outputs may be NULL; the others are what the full call returns"""
    import cetkmc
    L, nb = 9, 16
    theta, phi = TR.random_angles(L)
    lab = TR.labelling("scattered", L)
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, lab, theta, phi)
        e.import_clusters(lab)
        full = e.texture_profile(n_bins=nb, recluster=False)
        a, keep = _args(nb, TR.edges_cos(nb, 180.0), TR.edges_cos(nb, 90.0))
        for skip in TR.FIELDS + (None,):
            out = {k: np.full(full[k].shape, -7, np.int64) for k in TR.FIELDS}
            ptr = [None if k == skip else out[k].ctypes.data for k in TR.FIELDS]
            assert e.lib.cetkmc_texture_profile(e.h, C.byref(a), *ptr) == 0, e.error()
            for k in TR.FIELDS:
                assert (out[k] == -7).all() if k == skip else np.array_equal(out[k], full[k]), (skip, k)
        assert e.lib.cetkmc_texture_profile(e.h, C.byref(a), None, None, None) == 0
    finally:
        e.close()


def test_refusals():
    """every refusal is decided on the host: nothing is copied, the outputs are untouched, the lattice and the installed
    clustering are what they were"""
    import cetkmc
    L, nb = 8, 4
    theta, phi = TR.random_angles(L)
    lab = TR.labelling("scattered", L)
    ge, pe = TR.edges_cos(nb, 180.0), TR.edges_cos(nb, 90.0)
    out = {"gb_hist": np.full((L, 3, 64), -7, np.int64), "pole_hist": np.full((L, 64), -7, np.int64), "bad": np.full((L, 4), -7, np.int64)}
    ptr = [out[k].ctypes.data for k in TR.FIELDS]

    def refused(e, fn, handle, args, text):
        d2h = e.counters()["bytes_d2h"]
        a, keep = args
        assert fn(handle, None if a is None else C.byref(a), *ptr) != 0, text
        assert text in e.error(), (text, e.error())
        assert e.counters()["bytes_d2h"] == d2h and all((out[k] == -7).all() for k in TR.FIELDS), text

    e = cetkmc.Engine(L, n_slabs=2)
    try:
        _upload(e, L, lab, theta, phi)
        refused(e, e.lib.cetkmc_texture_profile, e.h, _args(nb, ge, pe), "one slab")
    finally:
        e.close()

    e = cetkmc.Engine(L)
    try:
        _upload(e, L, lab, theta, phi)
        one = e.lib.cetkmc_texture_profile
        refused(e, one, e.h, _args(nb, ge, pe), "preceding cetkmc_cluster")
        e.import_clusters(lab)
        keep = e.texture_profile(n_bins=nb, recluster=False)
        lattice = e.download()
        nan2, inf0, flat3, up1 = ge.copy(), pe.copy(), np.array([0.5, 0.2, 0.1, 0.1]), np.array([0.5, 0.6, 0.1])
        nan2[2], inf0[0] = np.nan, np.inf
        for args, text in [
            (_args(0, ge, pe), "n_bins 0 outside 1..64"), (_args(65, ge, pe), "n_bins 65 outside 1..64"),
            (_args(-3, None, None), "n_bins -3 outside 1..64"),
            (_args(nb, None, pe), "gb_edges is NULL"), (_args(nb, ge, None), "pole_edges is NULL"),
            (_args(nb, nan2, pe), "gb_edges[2] is not finite"), (_args(nb, ge, inf0), "pole_edges[0] is not finite"),
            (_args(5, flat3, flat3[::-1].copy()), "gb_edges[3] is not below its predecessor"),
            (_args(nb, ge, up1), "pole_edges[1] is not below its predecessor"),
            (_args(nb, ge, pe, (1.0, np.nan, 0.0)), "axis[1] is not finite"), (_args(nb, ge, pe, (1.0, 0.0, -np.inf)), "axis[2] is not finite"),
            ((None, None), "null argument"),
        ]:
            refused(e, one, e.h, args, text)
        refused(e, one, None, _args(nb, ge, pe), "null argument")
        refused(e, e.lib.cetkmc_ensemble_texture_profile, e.h, _args(nb, ge, pe), "not an ensemble handle")
        after = e.download()
        assert all(np.array_equal(lattice[k], after[k], equal_nan=True) for k in lattice)
        assert _bytes(e.texture_profile(n_bins=nb, recluster=False)) == _bytes(keep)       # still usable, same clustering
        assert TR.same(keep, _want(lab, theta, phi, nb)) == []
        one1 = e.texture_profile(n_bins=1, recluster=False)                                 # n_bins == 1 with NULL edges
        assert np.array_equal(one1["pole_hist"][:, 0], keep["pole_hist"].sum(axis=1))
    finally:
        e.close()
