"""cetkmc_grain_table against the NumPy comparator (grain_ref.py): every counter equal (integer sums, ==), the two angles of
the first voxel equal as int64 views.

Imported labellings (layer_ref.KINDS) reach the same-label side of the contact counts between face-adjacent rows and put
same-label and other-label stencil pairs across the kernel's wave, pass and block edges (64, 256 and 2048 voxels in row-major
order; grain_ref.check_import, pinned on the host in test_grain_ref_host.py).  The three regimes of the reduction by label:
one grain (every voxel has the same 18 destinations), singletons (nothing can be combined, far more labels in a block than
its table has slots) and the device clustering's own tables with thousands of grains beside one large one."""
import ctypes as C
import functools

import numpy as np
import pytest

import cluster_ref as CR
import grain_ref as GR
import layer_ref as LR

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(kind, L, seed):
    """labels (int32), state, theta, phi, size of an imported labelling (shared by the tests, read-only)"""
    raw, state = LR.labelling(kind, L, seed)
    lab, _, size, _ = LR.from_raw(raw)
    out = (lab.astype(np.int32), state) + GR.angles(L, L + seed) + (size,)
    for a in out:
        a.setflags(write=False)
    return out


def _upload(e, L, state, theta, phi):
    e.upload(state, theta, phi, np.full((L, L, L), 3000.0), np.zeros((L, L, L), np.int64))


def _stored(e):
    """the angles the device holds (the copies are compared with these, bit for bit)"""
    d = e.download(T=False)
    return d["state"], d["theta"], d["phi"]


def _imported(L, lab, state, theta, phi, size, calls=2):
    """the tables of ``calls`` calls on an import, the comparator's, and the bytes the first call copied"""
    import cetkmc
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state, theta, phi)
        tab = e.import_clusters(lab)
        assert np.array_equal(tab["size"], size)
        d2h = e.counters()["bytes_d2h"]
        got = [e.grain_table(recluster=False)]
        copied = e.counters()["bytes_d2h"] - d2h
        got += [e.grain_table(recluster=False) for _ in range(calls - 1)]
        st, th, ph = _stored(e)
    finally:
        e.close()
    assert np.array_equal(st, state)
    return got, GR.grain_ref(lab, state, th, ph), copied


@pytest.mark.parametrize("kind", LR.KINDS)
@pytest.mark.parametrize("L", GR.SHAPES)
def test_shapes(L, kind):
    lab, state, theta, phi, size = _case(kind, L, LR.case_seed(kind, L))
    got, want, copied = _imported(L, lab, state, theta, phi, size)
    GR.check_import(kind, L, lab, want)
    GR.check_identities(want, size)
    print(f"L={L} {kind}: grains {len(size)} largest {int(size.max()) if len(size) else 0} contacts {want['nb'].sum(axis=0).tolist()}")
    assert GR.same(got[0], want) == []
    assert GR.as_bytes(got[0]) == GR.as_bytes(got[1])
    assert copied == len(size) * GR.REC


def test_one_grain_129():
    """regime (a): every voxel of 129^3 adds to the same record"""
    L = 129
    raw, state = LR.one(L, 3)
    lab = raw.astype(np.int32)
    th, ph = GR.angles(L, 1)
    got, want, _ = _imported(L, lab, state, th, ph, np.array([L ** 3]))
    assert len(want["n"]) == 1 and int(want["n"][0]) == L ** 3 and int(want["sq"][0, 0]) == L * L * sum(i * i for i in range(L))
    assert GR.same(got[0], want) == [] and GR.as_bytes(got[0]) == GR.as_bytes(got[1])


def test_singletons_65():
    """regime (b): every occupied voxel is its own grain"""
    L = 65
    lab, state = GR.singletons(L)
    n = int(lab.max())
    th, ph = GR.angles(L, 2)
    got, want, copied = _imported(L, lab, state, th, ph, np.ones(n, np.int64))
    assert n > 100 * GR.SLOTS and (want["n"] == 1).all() and not want["nb"][:, 0].any() and want["nb"][:, 1].any()
    assert GR.same(got[0], want) == [] and GR.as_bytes(got[0]) == GR.as_bytes(got[1])
    assert copied == n * GR.REC


def test_labelled_voxels_of_state_0():
    """labels are not checked against the state: a labelled voxel whose state is 0 is in no species counter"""
    L = 9
    lab, _, theta, phi, size = _case("scattered", L, LR.case_seed("scattered", L))
    state = np.where(lab > 0, (np.arange(L ** 3).reshape(L, L, L) % 5), 3)
    got, want, _ = _imported(L, lab, state, theta, phi, size)
    assert (want["n_state"].sum(axis=1) < want["n"]).all() and want["n_state"].all()
    assert GR.same(got[0], want) == []


def _clustered(state, theta, phi, threshold, steps=0):
    """the table of the device clustering, the comparator's table from the independent clustering (cluster_ref) of what the
    device holds, and that clustering"""
    import cetkmc
    L = state.shape[0]
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state, theta, phi)
        d2h = e.counters()["bytes_d2h"]
        got = e.grain_table(threshold)
        copied = e.counters()["bytes_d2h"] - d2h
        again = e.grain_table(recluster=False)
        st, th, ph = _stored(e)
        sizes = e.clusters(threshold)["size"]
    finally:
        e.close()
    ref = CR.cluster_ref(st, th, ph, threshold)
    assert ref["ambiguous"] == 0
    want = GR.grain_ref(ref["labels"], st, th, ph)
    GR.check_identities(want, ref["size"])
    assert np.array_equal(sizes, ref["size"]) and copied == len(ref["size"]) * GR.REC
    assert GR.as_bytes(got) == GR.as_bytes(again)
    return got, want, ref


@pytest.mark.parametrize("L,fill,threshold,seed", [c for c in CR.GENERAL if c[0] <= 64] + [CR.GENERAL[4]])
def test_device_clustering(L, fill, threshold, seed):
    """regime (c) at L >= 64 and threshold 1.2: thousands of grains, one of which holds a large share"""
    state, theta, phi = CR.continuous(L, fill, seed)
    got, want, ref = _clustered(state, theta, phi, threshold)
    CR.check_general(ref, L, threshold)
    GR.check_clustered(want, largest=0.10 if (threshold == 1.2 and L >= 33) else None)
    print(f"L={L} thr={threshold}: grains {len(want['n'])} largest {want['n'].max() / want['n'].sum():.3f} "
          f"contacts {want['nb'].sum(axis=0).tolist()}")
    if (L, threshold) == (64, 1.2):
        assert len(want["n"]) == 10644 and 0.45 < want["n"].max() / want["n"].sum() < 0.47
    assert GR.same(got, want) == []


def test_textured_and_layer_identity():
    """the product's threshold on a textured lattice; the table's totals are the layer profile's"""
    import cetkmc
    state, theta, phi = CR.textured()
    got, want, ref = _clustered(state, theta, phi, 0.5)
    CR.check_textured(ref)
    GR.check_clustered(want, largest=0.10)
    assert GR.same(got, want) == []
    L = state.shape[0]
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state, theta, phi)
        lp = e.layer_profile(0.5)
        t = e.grain_table(recluster=False)
    finally:
        e.close()
    GR.check_identities(t, ref["size"], lp)
    assert GR.same(t, want) == []


def test_edge_lattice():
    """non-finite angles, also in first voxels: copied bit for bit"""
    state, theta, phi = CR.edge_lattice()
    got, want, ref = _clustered(state, theta, phi, 0.1)
    GR.check_clustered(want)
    assert not np.isfinite(want["first_theta"]).all() and not np.isfinite(want["first_phi"]).all()
    assert GR.same(got, want) == []


def test_after_stepping():
    """run_steps, then cluster and table, all queued on the handle's stream: the table of what a download shows"""
    import cetkmc
    import lattice_init
    L = 16
    np.random.seed(11)
    state, theta, phi, T, _ = lattice_init.initialize_lattice(lattice_size=L, n_seeds=6, impurity_c=0.1)
    e = cetkmc.Engine(L, impurity_c=0.1)
    try:
        e.upload(state, theta, phi, T, np.zeros((L, L, L), np.int64))
        before = e.grain_table()
        r = e.run_steps(0, 60, 0.0, None, None, None, rng_mode=2, seed=5, thermal_mode=1)
        assert r["done"] == 60 and r["status"] == 0
        got = e.grain_table()
        d = e.download()
        lab = e.clusters(0.5, labels=True)["labels"]
    finally:
        e.close()
    assert not np.array_equal(d["state"], state)
    want = GR.grain_ref(lab, d["state"], d["theta"], d["phi"])
    assert GR.same(got, want) == [] and GR.as_bytes(got) != GR.as_bytes(before)


def test_cap_and_unknown_count():
    import cetkmc
    L = 17
    lab, state = GR.singletons(L)
    theta, phi = GR.angles(L, 4)
    n = int(lab.max())
    assert n > 1100                                            # more grains than the first probe of Engine.grain_table
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state, theta, phi)
        e.import_clusters(lab)
        full = e.grain_table(recluster=False)
        want = GR.grain_ref(lab, state, *_stored(e)[1:])
        assert GR.same(full, want) == []
        rec = np.zeros(n, dtype=cetkmc.engine.GRAIN_DTYPE)
        for f in GR.FIELDS:
            rec[f] = full[f]
        for cap in (1, n // 2, n, n + 5):
            k = min(cap, n)
            buf = np.zeros(cap + 1, dtype=cetkmc.engine.GRAIN_DTYPE)
            buf["n"] = -7
            d2h = e.counters()["bytes_d2h"]
            assert e.lib.cetkmc_grain_table(e.h, cap, buf.ctypes.data) == 0
            assert e.counters()["bytes_d2h"] - d2h == k * GR.REC
            assert buf[:k].tobytes() == rec[:k].tobytes()
            assert (buf["n"][k:] == -7).all()
        for cap in (0, -3):                                    # as cetkmc_cluster_stats: nothing to do, also without a buffer
            d2h = e.counters()["bytes_d2h"]
            assert e.lib.cetkmc_grain_table(e.h, cap, None) == 0 and e.counters()["bytes_d2h"] == d2h
        e._cc_n = None                                         # a clustering the object does not know the size of
        assert GR.as_bytes(e.grain_table(recluster=False)) == GR.as_bytes(full)
    finally:
        e.close()


def test_refusals():
    import cetkmc
    L = 8
    lab, state, theta, phi, size = _case("blocks", L, LR.case_seed("blocks", L))
    n = len(size)
    buf = np.zeros(n + 1, dtype=cetkmc.engine.GRAIN_DTYPE)

    def refused(e, call, text):
        d2h = e.counters()["bytes_d2h"]
        assert call() != 0
        assert text in e.error(), e.error()
        assert e.counters()["bytes_d2h"] == d2h and not buf["n"].any()

    e = cetkmc.Engine(L, n_slabs=2)
    try:
        _upload(e, L, state, theta, phi)
        refused(e, lambda: e.lib.cetkmc_grain_table(e.h, n, buf.ctypes.data), "one slab")
    finally:
        e.close()
    e = cetkmc.Engine(L)
    try:
        _upload(e, L, state, theta, phi)
        refused(e, lambda: e.lib.cetkmc_grain_table(e.h, n, buf.ctypes.data), "cetkmc_grain_table needs a preceding cetkmc_cluster")
        with pytest.raises(RuntimeError, match="preceding cetkmc_cluster"):
            e.grain_table(recluster=False)
        e.import_clusters(lab)
        refused(e, lambda: e.lib.cetkmc_grain_table(e.h, n, None), "null argument")
        refused(e, lambda: e.lib.cetkmc_grain_table(None, n, buf.ctypes.data), "null")
        refused(e, lambda: e.lib.cetkmc_ensemble_grain_table(e.h, buf.ctypes.data), "not an ensemble handle")
        want = GR.grain_ref(lab, state, *_stored(e)[1:])
        assert GR.same(e.grain_table(recluster=False), want) == []             # the handle is still usable
        assert e.lib.cetkmc_struct_size(b"grain_rec") == GR.REC == C.sizeof(cetkmc._lib.GrainRec)
    finally:
        e.close()
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * 2)
    try:
        r0 = ens.replica(0)
        for r in range(2):
            _upload(ens.replica(r), L, state, theta, phi)
        refused(r0, lambda: ens.lib.cetkmc_ensemble_grain_table(ens.h, buf.ctypes.data), "needs a preceding cetkmc_ensemble_analyze")
        with pytest.raises(RuntimeError, match="cetkmc_ensemble_analyze"):
            ens.grain_table(recluster=False)
        ens.analyze(0.5, labels=False)
        refused(r0, lambda: ens.lib.cetkmc_ensemble_grain_table(ens.h, None), "null argument")
        refused(r0, lambda: ens.lib.cetkmc_grain_table(ens.h, n, buf.ctypes.data), "an ensemble handle goes to")
        with pytest.raises(RuntimeError, match="ensemble"):
            r0.grain_table()
        refused(r0, lambda: ens.lib.cetkmc_ensemble_grain_table(ens.replica(1).h, buf.ctypes.data), "not an ensemble handle")
        got = ens.grain_table(recluster=False)
        assert GR.as_bytes(got[0]) == GR.as_bytes(got[1]) and len(got[0]["n"]) > 0
    finally:
        ens.close()
