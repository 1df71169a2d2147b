"""cetkmc_ensemble_grain_table against the NumPy comparator (grain_ref.py) and against the same lattice on a single handle:
imported labellings with different grain counts per replica (an empty replica between others: a zero-length entry of the
concatenated table), the batched analysis of cluster_ref.ENSEMBLES, a frozen replica, the replica handle's own call."""
import numpy as np
import pytest

import cluster_ref as CR
import grain_ref as GR
import layer_ref as LR

pytestmark = pytest.mark.gpu


def _upload(e, L, state, theta, phi, T=None):
    e.upload(state, theta, phi, np.full((L, L, L), 3000.0) if T is None else T, np.zeros((L, L, L), np.int64))


@pytest.mark.parametrize("R,L", [(1, 8), (3, 9), (70, 8), (3, 33), (2, 65)])
def test_imports(R, L):
    import cetkmc
    empty = None if R == 1 else (0 if R <= 3 else R // 2)      # one replica with no grain at all (n = 0)
    cases = []
    for r in range(R):
        raw, state = LR.labelling(LR.KINDS[r % len(LR.KINDS)], L, r)
        lab = LR.from_raw(raw)[0].astype(np.int32)
        if r == empty:
            lab = np.zeros_like(lab)
        cases.append((lab, state) + GR.angles(L, 10 + r))
    labs = np.stack([c[0] for c in cases])
    n_cl = [int(c[0].max()) for c in cases]
    assert len(set(n_cl)) > 1 or R == 1, n_cl                  # different grain counts: the offsets matter
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * R)
    one = cetkmc.Engine(L)
    try:
        for r in range(R):
            _upload(ens.replica(r), L, *cases[r][1:])
        ens.analyze(0.5, labels=False)
        ens.import_clusters(labs)
        d2h = ens.replica(0).counters()["bytes_d2h"]
        got = ens.grain_table(recluster=False)
        assert ens.replica(0).counters()["bytes_d2h"] - d2h == sum(n_cl) * GR.REC
        again = ens.grain_table(recluster=False)
        assert [len(g["n"]) for g in got] == n_cl
        for r in range(R):
            lab, state = cases[r][:2]
            d = ens.replica(r).download(T=False)
            want = GR.grain_ref(lab, state, d["theta"], d["phi"])
            assert GR.same(got[r], want) == [], (R, L, r)
            assert GR.as_bytes(got[r]) == GR.as_bytes(again[r])
            if r < 8:
                _upload(one, L, state, d["theta"], d["phi"])   # the same import on a single handle
                one.import_clusters(lab)
                assert GR.as_bytes(one.grain_table(recluster=False)) == GR.as_bytes(got[r]), r
                if r > 0:                                      # the replica handle's own import (replica 0: the ensemble handle)
                    ens.replica(r).import_clusters(lab)
                    assert GR.as_bytes(ens.replica(r).grain_table(recluster=False)) == GR.as_bytes(got[r]), r
        if empty is not None:
            assert len(got[empty]["n"]) == 0 and len(got[empty + 1]["n"]) > 0
        assert all(GR.as_bytes(a) == GR.as_bytes(b) for a, b in zip(ens.grain_table(recluster=False), got))
    finally:
        one.close()
        ens.close()


@pytest.mark.parametrize("name", sorted(CR.ENSEMBLES))
def test_analyze(name):
    """the batched clustering's tables, the empty replica of L30_R6 between others included"""
    import cetkmc
    L, thresholds = CR.ENSEMBLES[name]
    lat = CR.ensemble_lattices(name)
    R = len(lat)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * R)
    one = cetkmc.Engine(L)
    try:
        for r, (st, th, ph, T) in enumerate(lat):
            _upload(ens.replica(r), L, st, th, ph, T)
        for thr in thresholds:
            got = ens.grain_table(thr)
            for r, (st, th, ph, _) in enumerate(lat):
                d = ens.replica(r).download(T=False)
                ref = CR.cluster_ref(d["state"], d["theta"], d["phi"], thr)
                CR.check_ensemble(name, r, st, ref)
                want = GR.grain_ref(ref["labels"], d["state"], d["theta"], d["phi"])
                GR.check_identities(want, ref["size"])
                if not (name == "L30_R6" and r in (2, 3)):      # (the empty replica and the one of singletons)
                    GR.check_clustered(want, full=(name == "L30_R6" and r == 1))
                assert GR.same(got[r], want) == [], (name, thr, r)
                if r == 1:                                     # the same lattice on a single handle, and the replica's own call
                    _upload(one, L, d["state"], d["theta"], d["phi"])
                    assert GR.as_bytes(one.grain_table(thr)) == GR.as_bytes(got[r])
                    assert GR.as_bytes(ens.replica(r).grain_table(thr)) == GR.as_bytes(got[r])
    finally:
        one.close()
        ens.close()


def test_frozen_replica_and_single_handle():
    import cetkmc
    import constants as K
    import test_gpu_layer_profile as TP
    L, R, fz = 8, 3, 1
    ramp = float(K.T_SUB) + (float(K.T_MELT) - float(K.T_SUB)) * (np.arange(L) / (L - 1))
    T = np.ascontiguousarray(np.broadcast_to(ramp[:, None, None], (L, L, L)))
    lat = [LR.random_blocks(L, 100 + r) + (T,) for r in range(R)]
    lat[fz] = TP._frozen_lattice(L, 99)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.05 * r) for r in range(R)])
    try:
        for r, (s, th, ph, Tr) in enumerate(lat):
            _upload(ens.replica(r), L, s, th, ph, Tr)
        res = ens.run(0, 2, 0.0, rng_mode=2, seeds=np.arange(R) + 3, thermal_mode=0)
        assert res["status"][fz] == 1 and res["done"][fz] == 0, "the frozen replica"
        an = ens.analyze(0.5, labels=True)
        got = ens.grain_table(recluster=False)
        for r in range(R):
            d = ens.replica(r).download(T=False)
            want = GR.grain_ref(an[r]["clusters"]["labels"], d["state"], d["theta"], d["phi"])
            GR.check_identities(want, an[r]["clusters"]["size"])
            assert GR.same(got[r], want) == [], r
        assert np.array_equal(ens.replica(fz).download(T=False)["state"], lat[fz][0]) and len(got[fz]["n"]) > 0
    finally:
        ens.close()
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, *lat[0][:3])
        e.clusters(0.5)
        buf = np.zeros(64, dtype=cetkmc.engine.GRAIN_DTYPE)
        assert e.lib.cetkmc_ensemble_grain_table(e.h, buf.ctypes.data) != 0 and "not an ensemble handle" in e.error()
        assert not buf["n"].any()
    finally:
        e.close()
