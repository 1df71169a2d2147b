"""cetkmc_layer_profile / cetkmc_ensemble_layer_profile on IMPORTED labellings (cetkmc_cluster_import /
cetkmc_ensemble_cluster_import) against the NumPy comparator (layer_ref.py): every counter equal (integer counting, ==).

The device clustering never puts two face neighbours into one grain, so with its labels every "neighbour has my label"
predicate of k_layer_profile has one value only (test_gpu_layer_profile.py).  Here the labellings come from the host --
one grain, slabs along each axis, one grain per random box, scattered disconnected grains, the constructed columnar /
equiaxed blocks -- and put same-grain and other-grain pairs across every tile, rim and plane-group edge of the kernel
(8 rows, 32 columns, 16 planes).  layer_ref.check_not_vacuous asserts that on the reference's inputs for every case
(test_layer_ref_host.py pins the fixed seeds on the host).

Also: the imported table and labels read back, a device clustering replacing an import and the reverse, ensembles (a
replica's rows = the comparator's = a single handle's = the replica handle's own import) and the refusals, every one of
which is decided on the host before anything reaches the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import layer_ref as LR

pytestmark = pytest.mark.gpu

REC = 144


def _ar():
    import constants as K
    return float(K.CET_AR_THRESHOLD)


@functools.lru_cache(maxsize=None)
def _case(kind, L, seed):
    """labels, state, first, size, bbox of a labelling (shared by the tests, read-only)"""
    raw, state = LR.labelling(kind, L, seed)
    out = LR.from_raw(raw)
    out = (out[0].astype(np.int32), state) + out[1:]
    for a in out:
        a.setflags(write=False)
    return out


def _upload(e, L, state):
    z = np.zeros((L, L, L))
    e.upload(state, z, z, np.full((L, L, L), 3000.0), np.zeros((L, L, L), np.int64))


def _bytes(p):
    return b"".join(np.ascontiguousarray(p[k]).tobytes() for k in LR.FIELDS)


def _table_equal(tab, first, size, bbox):
    return np.array_equal(tab["first"], first) and np.array_equal(tab["size"], size) and np.array_equal(tab["bbox"], bbox)


@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("L", LR.SHAPES)
def test_shapes(L, kind):
    import cetkmc
    import constants as K
    import metrics
    lab, state, first, size, bbox = _case(kind, L, LR.case_seed(kind, L))
    want = LR.layer_ref(lab, state, bbox, first, _ar())
    want_other = LR.layer_ref(lab, state, bbox, first, 1.5)
    LR.check_not_vacuous(kind, L, lab, want)
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state)
        tab = e.import_clusters(lab)
        d2h = e.counters()["bytes_d2h"]
        got = e.layer_profile(recluster=False)
        assert e.counters()["bytes_d2h"] - d2h == L * REC
        again = e.layer_profile(recluster=False)
        other = e.layer_profile(recluster=False, ar_threshold=1.5)
    finally:
        e.close()
    print(f"L={L} {kind}: grains {len(size)} n_occ {int(want['n_occ'].sum())} seg {want['seg'].sum(axis=0).tolist()} "
          f"cut {want['cut'].sum(axis=0).tolist()} gb {int(want['gb_state'].sum())} of {int(want['occ_state'].sum())}")
    assert _table_equal(tab, first, size, bbox)
    assert all(got[k].dtype == np.int64 and got[k].shape == want[k].shape for k in LR.FIELDS)
    assert LR.same(got, want) == []
    assert LR.same(other, want_other) == []
    assert _bytes(got) == _bytes(again)
    if kind == "constructed_blocks" and L >= 4:
        dx = float(K.VOXEL_SIZE)
        m, mw = metrics.layer_metrics(got, L, dx), metrics.layer_metrics(want, L, dx)
        assert m["InterceptRatio"] > 1.0
        assert [m[c] for c in metrics.LAYER_COLUMNS] == [mw[c] for c in metrics.LAYER_COLUMNS]
        if L >= 8:
            assert 0 < want["n_eq"].sum() < want["n_occ"].sum() and want_other["n_eq"].sum() < want["n_eq"].sum()


@pytest.mark.parametrize("L", (9, 33, 65))
def test_table_round_trip(L):
    """cluster_stats and cluster_labels after an import give from_raw's table and labels."""
    import cetkmc
    e = cetkmc.Engine(L)
    try:
        for kind in ("scattered", "blocks", "constructed_blocks"):
            lab, state, first, size, bbox = _case(kind, L, LR.case_seed(kind, L))
            if kind == "scattered":
                _upload(e, L, state)                            # the later imports: labels that are not those of the state
            assert _table_equal(e.import_clusters(lab), first, size, bbox), kind
            back = np.full((L, L, L), -1, np.int32)
            e._ck(e.lib.cetkmc_cluster_labels(e.h, back.ctypes.data))
            assert np.array_equal(back, lab), kind
            k = len(size) // 2                                  # a capped table: the first k grains
            f2, s2, b2 = np.zeros((max(k, 1), 3), np.int32), np.zeros(max(k, 1), np.int64), np.zeros((max(k, 1), 6), np.int32)
            e._ck(e.lib.cetkmc_cluster_stats(e.h, k, f2.ctypes.data, s2.ctypes.data, b2.ctypes.data))
            assert _table_equal(dict(first=f2[:k], size=s2[:k], bbox=b2[:k]), first[:k], size[:k], bbox[:k]), kind
    finally:
        e.close()


def test_replacement():
    """an import, then the device clustering in its place, then the import again: each profile is that of the labelling
    installed last, byte-identical on a repeated call.  The imported labels are not those of the lattice's state (occupancy
    from the labels, species from the state: the definition)."""
    import cetkmc
    import test_gpu_layer_profile as TP
    L = 17
    state, theta, phi = LR.random_blocks(L, 100 + L)
    lab, _, first, size, bbox = _case("scattered", L, LR.case_seed("scattered", L))
    assert not np.array_equal(lab != 0, state != 0)
    want_imp = LR.layer_ref(lab, state, bbox, first, _ar())
    e = cetkmc.Engine(L)
    try:
        TP._upload(e, L, state, theta, phi)
        e.import_clusters(lab)
        p1 = e.layer_profile(recluster=False)
        p2 = e.layer_profile(recluster=True)
        p2b = e.layer_profile(recluster=False)
        want_dev, cl, _ = TP._want(e)
        p2c = e.layer_profile(recluster=False)
        assert _table_equal(e.import_clusters(lab), first, size, bbox)
        p3 = e.layer_profile(recluster=False)
        p4 = e.layer_profile(recluster=False)
    finally:
        e.close()
    assert LR.same(p1, want_imp) == []
    assert LR.same(p2, want_dev) == [] and _bytes(p2) == _bytes(p2b) == _bytes(p2c)
    assert np.array_equal(p2["seg"], np.repeat(p2["n_occ"][:, None], 3, axis=1))     # the device's labels: no same-grain pair
    assert _bytes(p1) != _bytes(p2) and len(cl["size"]) != len(size)
    assert _bytes(p3) == _bytes(p1) == _bytes(p4)


@pytest.mark.parametrize("R,L", [(1, 8), (3, 9), (70, 8), (3, 33), (2, 65)])
def test_ensembles(R, L):
    import cetkmc
    empty = None if R == 1 else (0 if R <= 3 else R // 2)      # one replica with no grain at all (n = 0)
    cases = [_case(LR.KINDS[r % len(LR.KINDS)], L, r) for r in range(R)]
    labs = np.stack([c[0] for c in cases])
    if empty is not None:
        labs[empty] = 0
        z = np.zeros((0, 6), np.int64)
        cases[empty] = (labs[empty], cases[empty][1], z[:, :3], z[:, 0], z)
    n_cl = [len(c[3]) for c in cases]
    assert len(set(n_cl)) > 1 or R == 1, n_cl                  # different cluster counts: offs[r] + r matters
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * R)
    one = cetkmc.Engine(L)
    try:
        for r in range(R):
            _upload(ens.replica(r), L, cases[r][1])
        an = ens.analyze(0.5, labels=False)
        tabs = ens.import_clusters(labs)
        d2h = ens.replica(0).counters()["bytes_d2h"]
        got = ens.layer_profile(recluster=False)
        assert ens.replica(0).counters()["bytes_d2h"] - d2h == R * L * REC
        assert all(got[k].shape[:2] == (R, L) for k in LR.FIELDS)
        assert _bytes(got) == _bytes(ens.layer_profile(recluster=False))
        # the analysis data: the imported tables and labels, the replicas concatenated
        tot = sum(n_cl)
        f, s, b = np.zeros((max(tot, 1), 3), np.int32), np.zeros(max(tot, 1), np.int64), np.zeros((max(tot, 1), 6), np.int32)
        back = np.full((R, L, L, L), -1, np.int32)
        ens._ck(ens.lib.cetkmc_ensemble_analysis_data(ens.h, f.ctypes.data, s.ctypes.data, b.ctypes.data, back.ctypes.data, None, None))
        assert np.array_equal(back, labs)
        assert _table_equal(dict(first=f[:tot], size=s[:tot], bbox=b[:tot]), np.concatenate([c[2] for c in cases]),
                            np.concatenate([c[3] for c in cases]), np.concatenate([c[4] for c in cases]))
        for r in range(R):
            lab, state, first, size, bbox = cases[r]
            assert _table_equal(tabs[r], first, size, bbox), r
            mine = {k: got[k][r] for k in LR.FIELDS}
            assert LR.same(mine, LR.layer_ref(lab, state, bbox, first, _ar())) == [], (R, L, r)
            if r == empty:
                assert not any(mine[k].any() for k in LR.FIELDS) and an[r]["counts"][1:5].sum() > 0
            _upload(one, L, state)                             # the same import on a single handle
            one.import_clusters(lab)
            assert _bytes(one.layer_profile(recluster=False)) == _bytes(mine), r
            if r > 0:                                          # the replica handle's own import (replica 0: the ensemble handle)
                assert _table_equal(ens.replica(r).import_clusters(lab), first, size, bbox), r
                assert _bytes(ens.replica(r).layer_profile(recluster=False)) == _bytes(mine), r
        with pytest.raises(RuntimeError, match="ensemble"):
            ens.replica(0).import_clusters(labs[0])
        assert _bytes(ens.layer_profile(recluster=False)) == _bytes(got)      # the batched import is still the one installed
        again = ens.analyze(0.5, labels=False)                 # a later analysis replaces the import
        assert [len(a["clusters"]["size"]) for a in again] == [len(a["clusters"]["size"]) for a in an]
    finally:
        one.close()
        ens.close()


def _refused(e, call, text, keep):
    """one refusal: rc != 0, the message, nothing copied to the host, the installed clustering still gives its profile"""
    d2h = e.counters()["bytes_d2h"]
    assert call() != 0
    assert text in e.error(), e.error()
    assert e.counters()["bytes_d2h"] == d2h
    if keep is not None:
        assert _bytes(e.layer_profile(recluster=False)) == keep, text


def test_refusals():
    import cetkmc
    L = 8
    lab, state, first, size, bbox = _case("blocks", L, LR.case_seed("blocks", L))
    n = len(size)
    assert n >= 3
    nc = C.c_int64(-7)

    def bad_labels(kind):
        x = np.array(lab)
        if kind == "beyond":                                   # label n + 1 where id 1 is due
            x[tuple(first[0])] = n + 1
            return x, tuple(first[0])
        if kind == "negative":
            x[3, 2, 1] = -1
            return x, (3, 2, 1)
        if kind == "gap":                                      # id 2 absent: id 3 comes where 2 is due
            x[x == 2] = 0
            return x, tuple(first[2])
        x[lab == 1], x[lab == 2] = 2, 1                        # ids 1 and 2 swapped: not in first-occurrence order
        return x, tuple(first[0])

    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state)

        def imp(x, out=nc):
            return e.lib.cetkmc_cluster_import(e.h, None if x is None else x.ctypes.data, None if out is None else C.byref(out))
        _refused(e, lambda: imp(None), "null argument", None)
        with pytest.raises(RuntimeError, match="preceding cetkmc_cluster"):
            e.layer_profile(recluster=False)                   # a refused import installs nothing
        e.import_clusters(lab)
        keep = _bytes(e.layer_profile(recluster=False))
        assert LR.same(e.layer_profile(recluster=False), LR.layer_ref(lab, state, bbox, first, _ar())) == []
        for kind in ("beyond", "negative", "gap", "swapped"):
            x, at = bad_labels(kind)
            _refused(e, lambda: imp(x), f"at voxel ({at[0]}, {at[1]}, {at[2]})", keep)
            assert f"label {int(x[at])} " in e.error()
        _refused(e, lambda: imp(None), "null argument", keep)
        _refused(e, lambda: imp(np.array(lab), None), "null argument", keep)
        _refused(e, lambda: e.lib.cetkmc_cluster_import(None, lab.ctypes.data, C.byref(nc)), "null argument", keep)
        _refused(e, lambda: e.lib.cetkmc_ensemble_cluster_import(e.h, lab.ctypes.data, C.byref(nc)), "not an ensemble handle", keep)
        assert nc.value == -7
    finally:
        e.close()

    e = cetkmc.Engine(L, n_slabs=2)
    try:
        _upload(e, L, state)
        _refused(e, lambda: e.lib.cetkmc_cluster_import(e.h, lab.ctypes.data, C.byref(nc)), "one slab", None)
    finally:
        e.close()

    R = 3
    labs = np.stack([lab] * R)
    ncs = np.full(R, -7, np.int64)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * R)
    try:
        r0 = ens.replica(0)
        for r in range(R):
            _upload(ens.replica(r), L, state)

        def eimp(x):
            return ens.lib.cetkmc_ensemble_cluster_import(ens.h, None if x is None else x.ctypes.data, ncs.ctypes.data)
        _refused(r0, lambda: eimp(labs), "needs a preceding cetkmc_ensemble_analyze", None)
        ens.analyze(0.5, labels=False)
        keep = _bytes(ens.layer_profile(recluster=False))

        def check(call, text):
            _refused(r0, call, text, None)
            assert _bytes(ens.layer_profile(recluster=False)) == keep, text
        for kind in ("beyond", "negative", "gap", "swapped"):  # one bad replica of three
            x, at = bad_labels(kind)
            bad = np.stack([lab, x, lab])
            check(lambda: eimp(bad), f"at voxel ({at[0]}, {at[1]}, {at[2]}) of replica 1")
        check(lambda: eimp(None), "null argument")
        check(lambda: ens.lib.cetkmc_ensemble_cluster_import(ens.h, labs.ctypes.data, None), "null argument")
        check(lambda: ens.lib.cetkmc_cluster_import(ens.h, lab.ctypes.data, C.byref(nc)), "an ensemble handle goes to")
        assert (ncs == -7).all() and nc.value == -7
        ens.import_clusters(labs)                              # still usable
        got = ens.layer_profile(recluster=False)
        want = LR.layer_ref(lab, state, bbox, first, _ar())
        assert all(LR.same({k: got[k][r] for k in LR.FIELDS}, want) == [] for r in range(R)) and _bytes(got) != keep
    finally:
        ens.close()
