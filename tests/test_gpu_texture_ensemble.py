"""cetkmc_ensemble_texture_profile: the batched rows of every replica equal the replica's single-handle rows and the NumPy
comparator (texture_ref.py), on the device's own analysis and on imported labellings, with distinct lattices and labellings
per replica and one replica frozen; the handle-kind refusals.  As in test_gpu_texture_profile.py every comparison is ==
after the comparator's values were found clear of the edges."""
import ctypes as C

import numpy as np
import pytest

import texture_ref as TR

pytestmark = pytest.mark.gpu

L, R, NB = 33, 5, 16
AXIS = (0.5, -1.0, 0.25)


def _bytes(p):
    return b"".join(np.ascontiguousarray(p[k]).tobytes() for k in TR.FIELDS)


def _frozen_lattice(seed):
    """No event is possible (defect voxels and empty ones only, plane L-1 full, every T within delta_T_c of T_melt): the
    replica terminates in its first step and is frozen."""
    import constants as K
    rs = np.random.RandomState(seed)
    state = np.where(rs.random_sample((L, L, L)) < 0.5, 4, 0).astype(np.int64)
    state[L - 1] = 4
    return state, float(K.T_MELT) - 5.0 * rs.random_sample((L, L, L))


def _want(lab, theta, phi):
    ge, pe = TR.edges_cos(NB, 180.0), TR.edges_cos(NB, 90.0)
    values = (TR.face_values(lab, theta, phi), TR.pole_values(lab, theta, phi, AXIS))
    assert TR.n_ambiguous(values, ge, pe) == 0
    return TR.texture_ref(lab, theta, phi, ge, pe, AXIS, values=values)


def test_batched_rows():
    import cetkmc
    import constants as K
    fz = 2
    labs = np.stack([TR.labelling(TR.KINDS[r], L) for r in range(R)])
    ramp = float(K.T_SUB) + (float(K.T_MELT) - float(K.T_SUB)) * (np.arange(L) / (L - 1))
    zi = np.zeros((L, L, L), np.int64)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.05 * r) for r in range(R)])
    one = cetkmc.Engine(L)
    try:
        for r in range(R):
            theta, phi = TR.random_angles(L, s=r)
            state, T = np.where(labs[r] != 0, 1 + r % 3, 0).astype(np.int64), np.ascontiguousarray(np.broadcast_to(ramp[:, None, None], (L, L, L)))
            if r == fz:
                state, T = _frozen_lattice(99)
            ens.replica(r).upload(state, theta, phi, T, zi)
        res = ens.run(0, 2, 0.0, rng_mode=2, seeds=np.arange(R) + 3, thermal_mode=0)
        assert res["status"][fz] == 1 and res["done"][fz] == 0, "the frozen replica"
        with pytest.raises(RuntimeError, match="cetkmc_ensemble_analyze"):
            ens.texture_profile(n_bins=NB, axis=AXIS, recluster=False)
        an = ens.analyze(0.5, labels=True)
        d2h = ens.replica(0).counters()["bytes_d2h"]
        dev = ens.texture_profile(n_bins=NB, axis=AXIS, recluster=False)          # the device's own clustering
        assert ens.replica(0).counters()["bytes_d2h"] - d2h == R * L * (4 * NB + 4) * 8
        assert dev["gb_hist"].shape == (R, L, 3, NB) and dev["pole_hist"].shape == (R, L, NB) and dev["bad"].shape == (R, L, 4)
        assert _bytes(dev) == _bytes(ens.texture_profile(n_bins=NB, axis=AXIS, recluster=False))
        fields = [ens.replica(r).download() for r in range(R)]
        for r in range(R):
            mine = {k: dev[k][r] for k in TR.FIELDS}
            assert TR.same(mine, _want(an[r]["clusters"]["labels"], fields[r]["theta"], fields[r]["phi"])) == [], r
        ens.import_clusters(labs)                                                   # the caller's labellings in its place
        got = ens.texture_profile(n_bins=NB, axis=AXIS, recluster=False)
        layer = ens.layer_profile(recluster=False)
        sums = set()
        for r in range(R):
            d = fields[r]
            mine = {k: got[k][r] for k in TR.FIELDS}
            assert TR.same(mine, _want(labs[r], d["theta"], d["phi"])) == [], r
            assert np.array_equal(mine["gb_hist"].sum(axis=2) + mine["bad"][:, :3], layer["cut"][r])
            assert np.array_equal(mine["pole_hist"].sum(axis=1) + mine["bad"][:, 3], layer["n_occ"][r])
            assert mine["gb_hist"].sum() > 0 and _bytes(mine) != _bytes({k: dev[k][r] for k in TR.FIELDS})
            sums.add(_bytes(mine))
            one.upload(d["state"], d["theta"], d["phi"], d["T"], zi)               # the same lattice on a single handle
            one.import_clusters(labs[r])
            assert _bytes(one.texture_profile(n_bins=NB, axis=AXIS, recluster=False)) == _bytes(mine), r
            if r > 0:                                          # the replica handle's own call (replica 0: the ensemble handle)
                ens.replica(r).import_clusters(labs[r])
                assert _bytes(ens.replica(r).texture_profile(n_bins=NB, axis=AXIS, recluster=False)) == _bytes(mine), r
        assert len(sums) == R                                  # the replicas do hold different lattices
        assert np.array_equal(fields[fz]["state"], _frozen_lattice(99)[0])
        with pytest.raises(RuntimeError, match="ensemble"):
            ens.replica(0).texture_profile(n_bins=NB, recluster=False)
        assert _bytes(ens.texture_profile(n_bins=NB, axis=AXIS, recluster=False)) == _bytes(got)      # still usable
    finally:
        one.close()
        ens.close()


def test_handle_kinds():
    import cetkmc
    from cetkmc import _lib
    Ls = 8
    theta, phi = TR.random_angles(Ls)
    lab = TR.labelling("scattered", Ls)
    state = np.where(lab != 0, 1, 0).astype(np.int64)
    T, zi = np.full((Ls, Ls, Ls), 3000.0), np.zeros((Ls, Ls, Ls), np.int64)
    a = _lib.TextureArgs()
    a.n_bins = 1
    a.axis[:] = (1.0, 0.0, 0.0)
    pole = np.full((2, Ls, 1), -7, np.int64)
    e = cetkmc.Engine(Ls)
    try:
        e.upload(state, theta, phi, T, zi)
        e.import_clusters(lab)
        assert e.lib.cetkmc_ensemble_texture_profile(e.h, C.byref(a), None, pole.ctypes.data, None) != 0
        assert "not an ensemble handle" in e.error()
    finally:
        e.close()
    ens = cetkmc.Ensemble(Ls, [cetkmc.default_params(0.0)] * 2)
    try:
        for r in range(2):
            ens.replica(r).upload(state, theta, phi, T, zi)
        d2h = ens.replica(0).counters()["bytes_d2h"]
        assert ens.lib.cetkmc_ensemble_texture_profile(ens.h, C.byref(a), None, pole.ctypes.data, None) != 0
        assert "cetkmc_ensemble_analyze" in ens.error()
        ens.analyze(0.5, labels=False)
        d2h = ens.replica(0).counters()["bytes_d2h"]
        assert ens.lib.cetkmc_texture_profile(ens.h, C.byref(a), None, pole.ctypes.data, None) != 0
        assert "an ensemble handle goes to" in ens.error()
        assert ens.lib.cetkmc_ensemble_texture_profile(ens.h, None, None, pole.ctypes.data, None) != 0 and "null argument" in ens.error()
        assert ens.replica(0).counters()["bytes_d2h"] == d2h and (pole == -7).all()
        assert ens.lib.cetkmc_ensemble_texture_profile(ens.h, C.byref(a), None, pole.ctypes.data, None) == 0, ens.error()
        assert (pole.sum(axis=(1, 2)) == np.count_nonzero(state)).all()                # n_bins == 1: every occupied voxel
    finally:
        ens.close()
