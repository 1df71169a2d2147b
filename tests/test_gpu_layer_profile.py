"""cetkmc_layer_profile / cetkmc_ensemble_layer_profile against the NumPy comparator (layer_ref.py), evaluated on the labels,
the per-grain table and the state downloaded from the same handle: every counter equal (integer counting, asserted with ==).
Shapes across every tile edge (8 rows, 32 columns, 16 planes), constructed / random / full / empty lattices, determinism, the
stream ordering behind stepping work, ensembles (a replica's rows = the comparator's = a single handle's = the replica
handle's own call) and the refusals.

Replica 0's handle IS the ensemble handle, which the single call refuses by definition: the replica-handle comparison covers
the replicas r >= 1.

What the device clustering cannot produce: two face neighbours in one grain (its 14-stencil keeps the parity of i + j + k),
so with its labels seg[a] == n_occ and the "neighbour has my label" side of the predicates is not reached in this file:
test_gpu_layer_imported.py reaches it on the device through imported labellings (cetkmc_cluster_import), and
test_layer_ref_host.py pins the comparator on the host."""
import numpy as np
import pytest

import layer_ref as LR

pytestmark = pytest.mark.gpu

SHAPES = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 129)
KINDS = ("constructed", "random", "full", "empty")
REC = 144


def _ar():
    import constants as K
    return float(K.CET_AR_THRESHOLD)


def _lattice(kind, L, seed=0):
    if kind == "constructed":
        return LR.constructed(L, species=np.random.RandomState(7 + L + seed))[:3]
    if kind == "random":
        return LR.random_blocks(L, 100 + L + seed)
    z = np.zeros((L, L, L))
    return np.full((L, L, L), 2 if kind == "full" else 0, np.int64), z, z


def _upload(e, L, state, theta, phi):
    e.upload(state, theta, phi, np.full((L, L, L), 3000.0), np.zeros((L, L, L), np.int64))


def _want(e, ar=None):
    """the comparator on what the handle holds: its last clustering (labels, first voxels, bounding boxes) and its state"""
    cl = e.clusters(0.5, labels=True)
    state = e.download(theta=False, phi=False, T=False)["state"]
    assert np.array_equal(cl["labels"] != 0, state != 0)
    return LR.layer_ref(cl["labels"], state, cl["bbox"], cl["first"], _ar() if ar is None else ar), cl, state


def _bytes(p):
    return b"".join(np.ascontiguousarray(p[k]).tobytes() for k in LR.FIELDS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L", SHAPES)
def test_shapes(L, kind):
    import cetkmc
    state, theta, phi = _lattice(kind, L)
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state, theta, phi)
        want, cl, _ = _want(e)
        d2h = e.counters()["bytes_d2h"]
        got = e.layer_profile(recluster=False)
        assert e.counters()["bytes_d2h"] - d2h == L * REC
        again = e.layer_profile(recluster=False)
        other = e.layer_profile(recluster=False, ar_threshold=1.5)
        want_other = LR.layer_ref(cl["labels"], state, cl["bbox"], cl["first"], 1.5)
    finally:
        e.close()
    print(f"L={L} {kind}: grains {len(cl['size'])} n_occ {int(want['n_occ'].sum())} n_eq {int(want['n_eq'].sum())} "
          f"cut {want['cut'].sum(axis=0).tolist()} gb {want['gb_state'].sum(axis=0).tolist()}")
    assert all(got[k].dtype == np.int64 and got[k].shape == want[k].shape for k in LR.FIELDS)
    assert LR.same(got, want) == []
    assert LR.same(other, want_other) == []
    assert _bytes(got) == _bytes(again)
    assert got["n_occ"].sum() == np.count_nonzero(state) and got["n_start"].sum() == len(cl["size"])
    if kind == "empty":
        assert not any(got[k].any() for k in LR.FIELDS)
    elif L >= 8:                                               # guards against a vacuous pass
        assert all(want["cut"][:, a].sum() > 0 for a in range(3))
        if kind == "constructed":
            assert 0 < want["n_eq"].sum() < want["n_occ"].sum()
            assert want_other["n_eq"].sum() < want["n_eq"].sum()
        if kind == "random":
            assert all(want["gb_state"][:, t].sum() > 0 for t in range(4))
            assert set(np.unique(state)) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("thermal_mode", (1, 2))
def test_after_stepping(thermal_mode):
    """run_steps, then cluster, then profile, all queued on the handle's stream: the profile of what a download shows."""
    import cetkmc
    import lattice_init
    from thermal_solver import laser_scan_planes
    L = 16
    np.random.seed(11)
    state, theta, phi, T, _ = lattice_init.initialize_lattice(lattice_size=L, n_seeds=6, impurity_c=0.1)
    e = cetkmc.Engine(L, impurity_c=0.1)
    try:
        e.upload(state, theta, phi, T, np.zeros((L, L, L), np.int64))
        before = e.layer_profile()
        q = laser_scan_planes(L, dict(power=200.0, start=4.0, speed=1.0), 0, 60) if thermal_mode == 2 else None
        r = e.run_steps(0, 60, 0.0, None, None, None, rng_mode=2, seed=5, thermal_mode=thermal_mode, q_planes=q)
        assert r["done"] == 60 and r["status"] == 0
        got = e.layer_profile()                                # clusters, then profiles, behind the steps
        want, _, now = _want(e)
    finally:
        e.close()
    assert not np.array_equal(now, state)
    assert LR.same(got, want) == [] and _bytes(got) != _bytes(before)


def _frozen_lattice(L, seed):
    """No event is possible (defect voxels and empty ones only, plane L-1 full, every T within delta_T_c of T_melt): the
    replica terminates in its first step and is frozen."""
    import constants as K
    rs = np.random.RandomState(seed)
    state = np.where(rs.random_sample((L, L, L)) < 0.5, 4, 0).astype(np.int64)
    state[L - 1] = 4
    th = np.arccos(rs.uniform(-1, 1, (L, L, L)))
    return state, th, rs.uniform(-np.pi, np.pi, (L, L, L)), float(K.T_MELT) - 5.0 * rs.random_sample((L, L, L))


@pytest.mark.parametrize("R,L", [(1, 8), (3, 8), (70, 8), (3, 33), (4, 128)])
def test_ensembles(R, L):
    import cetkmc
    import constants as K
    ramp = float(K.T_SUB) + (float(K.T_MELT) - float(K.T_SUB)) * (np.arange(L) / max(L - 1, 1))
    T = np.ascontiguousarray(np.broadcast_to(ramp[:, None, None], (L, L, L)))
    lat = [_lattice(("random", "constructed")[r % 2], L, seed=r) + (T,) for r in range(R)]
    fz = R // 2
    lat[fz] = _frozen_lattice(L, 99)
    zi = np.zeros((L, L, L), np.int64)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.05 * (r % 4)) for r in range(R)])
    one = cetkmc.Engine(L)
    try:
        for r, (s, th, ph, Tr) in enumerate(lat):
            ens.replica(r).upload(s, th, ph, Tr, zi)
        res = ens.run(0, 2, 0.0, rng_mode=2, seeds=np.arange(R) + 3, thermal_mode=0)
        assert res["status"][fz] == 1 and res["done"][fz] == 0, "the frozen replica"
        an = ens.analyze(0.5, labels=True)
        d2h = ens.replica(0).counters()["bytes_d2h"]
        got = ens.layer_profile(recluster=False)
        assert ens.replica(0).counters()["bytes_d2h"] - d2h == R * L * REC
        assert all(got[k].shape[:2] == (R, L) for k in LR.FIELDS)
        again = ens.layer_profile(recluster=False)
        assert _bytes(got) == _bytes(again)
        sums = set()
        for r in range(R):
            d = ens.replica(r).download()
            cl = an[r]["clusters"]
            mine = {k: got[k][r] for k in LR.FIELDS}
            want = LR.layer_ref(cl["labels"], d["state"], cl["bbox"], cl["first"], _ar())
            assert LR.same(mine, want) == [], (R, L, r)
            if r == fz:
                assert np.array_equal(d["state"], lat[fz][0]) and want["n_occ"].sum() > 0
            sums.add(_bytes(mine))
            if r > 0 and (L < 128 or r == 1):                 # the replica handle's own call (replica 0: the ensemble handle)
                assert _bytes(ens.replica(r).layer_profile()) == _bytes(mine), r
            if L < 128 or r == 1:                             # the same lattice on a single handle
                one.upload(d["state"], d["theta"], d["phi"], d["T"], zi)
                assert _bytes(one.layer_profile()) == _bytes(mine), r
        assert len(sums) == R or R > 8                        # the replicas do hold different lattices
        with pytest.raises(RuntimeError, match="ensemble"):
            ens.replica(0).layer_profile()
        assert _bytes(ens.layer_profile(recluster=False)) == _bytes(got)      # still usable, and the analysis is still there
    finally:
        one.close()
        ens.close()


def test_refusals():
    import cetkmc
    L = 8
    state, theta, phi = _lattice("random", L)
    buf = np.zeros(L, dtype=cetkmc.engine.LAYER_DTYPE)
    e = cetkmc.Engine(L, n_slabs=2)
    try:
        _upload(e, L, state, theta, phi)
        d2h = e.counters()["bytes_d2h"]
        assert e.lib.cetkmc_layer_profile(e.h, 3.0, buf.ctypes.data) != 0 and "one slab" in e.error()
        assert e.counters()["bytes_d2h"] == d2h
    finally:
        e.close()
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state, theta, phi)
        d2h = e.counters()["bytes_d2h"]
        with pytest.raises(RuntimeError, match="preceding cetkmc_cluster"):
            e.layer_profile(recluster=False)
        want, _, _ = _want(e)
        d2h = e.counters()["bytes_d2h"]
        assert e.lib.cetkmc_layer_profile(e.h, 3.0, None) != 0 and e.error()
        assert e.lib.cetkmc_ensemble_layer_profile(e.h, 3.0, buf.ctypes.data) != 0 and "ensemble" in e.error()
        assert e.counters()["bytes_d2h"] == d2h and not buf["n_occ"].any()
        assert LR.same(e.layer_profile(recluster=False), want) == []          # the handle is still usable
    finally:
        e.close()
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * 2)
    try:
        for r in range(2):
            _upload(ens.replica(r), L, state, theta, phi)
        big = np.zeros((2, L), dtype=cetkmc.engine.LAYER_DTYPE)
        assert ens.lib.cetkmc_ensemble_layer_profile(ens.h, 3.0, big.ctypes.data) != 0 and "cetkmc_ensemble_analyze" in ens.error()
        ens.analyze(0.5, labels=False)
        assert ens.lib.cetkmc_ensemble_layer_profile(ens.h, 3.0, None) != 0 and ens.error()
        assert ens.lib.cetkmc_layer_profile(ens.h, 3.0, buf.ctypes.data) != 0 and "ensemble" in ens.error()
        assert not buf["n_occ"].any() and not big["n_occ"].any()
        got = ens.layer_profile(recluster=False)
        assert _bytes({k: got[k][0] for k in LR.FIELDS}) == _bytes({k: got[k][1] for k in LR.FIELDS})
        assert got["n_occ"].sum() == 2 * np.count_nonzero(state)
    finally:
        ens.close()
