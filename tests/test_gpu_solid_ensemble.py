"""cetkmc_ensemble_solid_begin / _update / _profile and the replica handles' read and profile: against the NumPy comparator
(solid_ref.py) for every replica, and byte for byte against the same lattices on a single handle.  The replicas differ (own
sequences of states and temperatures, own labellings with different grain counts); one is empty throughout (no record, a
zero-length entry of the concatenated grain records) and one is frozen (terminated in a step before the maps began: nothing
changes in it).  The launch sequence of the three batched calls is fixed in the host code (one memset pair and one launch,
one launch, two launches) whatever R."""
import numpy as np
import pytest

import layer_ref as LR
import solid_ref as SR
import test_gpu_layer_profile as TP

pytestmark = pytest.mark.gpu

SCALES = SR.GRID_SCALES
STAMPS = (0, 20, 4000000000)
DTS = (1.0, 0.5, 4.0)


def _map_bytes(m):
    return b"".join(np.ascontiguousarray(m[k]).tobytes() for k in ("stamp",) + SR.MAP_FIELDS)


def _rec_bytes(p):
    return b"".join(np.ascontiguousarray(p[k]).tobytes() for k in SR.FIELDS)


def _up(e, L, st, T, full):
    if full:
        z = np.zeros((L, L, L))
        e.upload(st, z, z, T, np.zeros((L, L, L), np.int64))
    else:
        e.upload(state=st, T=T)


@pytest.mark.parametrize("R,L", [(1, 30), (3, 30), (70, 30), (4, 64)])
def test_ensembles(R, L):
    import cetkmc
    empty = None if R == 1 else 0
    fz = None if R < 3 else 1
    seqs, labs = [], []
    for r in range(R):
        seq = SR.sequence(L, 100 + r)
        if r == empty:
            seq = [(np.zeros_like(st), T) for st, T in seq]
        if r == fz:
            st, _, _, T = TP._frozen_lattice(L, 99)
            seq = [(st, T)] + [(st, SR.grid_T(L, 7 + u)) for u in range(3)]     # only its T moves (no state upload: stays frozen)
        seqs.append(seq)
        raw, _ = LR.labelling(LR.KINDS[r % len(LR.KINDS)], L, r)
        labs.append(np.zeros((L, L, L), np.int32) if r == empty else LR.from_raw(raw)[0].astype(np.int32))
    n_cl = [int(l.max()) for l in labs]
    assert R == 1 or len(set(n_cl)) > 1
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.02 * (r % 5)) for r in range(R)])
    one = cetkmc.Engine(L)
    try:
        for r in range(R):
            _up(ens.replica(r), L, *seqs[r][0], True)
        if fz is not None:
            res = ens.run(0, 1, 0.0, rng_mode=2, seeds=np.arange(R) + 3, thermal_mode=0)
            assert res["status"][fz] == 1 and res["done"][fz] == 0, "the frozen replica"
            for r in range(R):
                if r != fz:
                    _up(ens.replica(r), L, *seqs[r][0], True)              # the lattices the step changed, as they were
        ens.solid_begin()
        refs = [SR.SolidRef(*seqs[r][0]) for r in range(R)]
        for u in range(3):
            for r in range(R):
                if r == fz:
                    ens.replica(r).upload(T=seqs[r][u + 1][1])
                else:
                    _up(ens.replica(r), L, *seqs[r][u + 1], False)
            info = ens.solid_update(STAMPS[u], DTS[u], 1.0)
            for r in range(R):
                want = refs[r].update(*seqs[r][u + 1], STAMPS[u], 1.0, DTS[u])
                assert {k: int(info[k][r]) for k in info} == want, (R, L, u, r)
        if fz is not None:
            res = ens.run(0, 1, 0.0, rng_mode=2, seeds=np.arange(R) + 3, thermal_mode=0)
            assert res["status"][fz] == 1 and res["done"][fz] == 0, "still frozen"
            assert int(info["n_recorded"][fz]) == 0 and int(info["n_recorded"][empty]) == 0 and int(info["n_recorded"][2]) > 0
            for r in range(R):
                if r != fz:
                    _up(ens.replica(r), L, *seqs[r][3], False)
            info = ens.solid_update(5, 1.0, 1.0)
            for r in range(R):
                assert {k: int(info[k][r]) for k in info} == refs[r].update(*seqs[r][3], 5, 1.0, 1.0), r
        assert all(ref.ties(SCALES) == 0 for ref in refs)
        ens.analyze(0.5, labels=False)
        ens.import_clusters(np.stack(labs))
        d2h = ens.replica(0).counters()["bytes_d2h"]
        got = ens.solid_profile(SCALES, grains=True, recluster=False)
        assert ens.replica(0).counters()["bytes_d2h"] - d2h == (R * L + sum(n_cl)) * SR.REC
        plain = ens.solid_profile(SCALES)
        assert plain["grains"] is None and _rec_bytes(plain["layers"]) == _rec_bytes(got["layers"])
        assert [len(g["n_rec"]) for g in got["grains"]] == n_cl
        for r in range(R):
            want = refs[r].profile(SCALES, labs[r])
            SR.check_identities(refs[r], want, SCALES, labs[r])
            lay = {k: got["layers"][k][r] for k in SR.FIELDS}
            assert SR.same_records(lay, want["layers"]) == [] and SR.same_records(got["grains"][r], want["grains"]) == [], (R, L, r)
            m = ens.solid_read(r)
            assert SR.same_map(m, refs[r].map()) == [], (R, L, r)
            if r < 6 and r != fz:
                # the same lattice on a single handle: begin (a second begin from the second replica on), the same updates
                _up(one, L, *seqs[r][0], True)
                one.solid_begin()
                for u in range(3):
                    _up(one, L, *seqs[r][u + 1], False)
                    one.solid_update(STAMPS[u], DTS[u], 1.0)
                if fz is not None:
                    one.solid_update(5, 1.0, 1.0)
                assert _map_bytes(one.solid_read()) == _map_bytes(m), r
                one.import_clusters(labs[r])
                p1 = one.solid_profile(SCALES, grains=True, recluster=False)
                assert _rec_bytes(p1["layers"]) == _rec_bytes(lay) and _rec_bytes(p1["grains"]) == _rec_bytes(got["grains"][r]), r
                if r > 0:              # the replica handle's own profile, from its own import (replica 0: the ensemble handle)
                    ens.replica(r).import_clusters(labs[r])
                    pr = ens.replica(r).solid_profile(SCALES, grains=True, recluster=False)
                    assert _rec_bytes(pr["layers"]) == _rec_bytes(lay) and _rec_bytes(pr["grains"]) == _rec_bytes(got["grains"][r]), r
        if empty is not None:
            assert len(got["grains"][empty]["n_rec"]) == 0 and not got["layers"]["n_rec"][empty].any()
            assert (got["layers"]["stamp_min"][empty] == SR.NONE_MIN).all()
        ens.solid_begin()                                                  # a second begin resets every replica's map
        assert all((ens.solid_read(r)["stamp"] == -1).all() for r in range(min(R, 3)))
        ens.solid_end()
        with pytest.raises(RuntimeError, match="needs a map"):
            ens.solid_read(0)
    finally:
        one.close()
        ens.close()
