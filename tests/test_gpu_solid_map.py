"""cetkmc_solid_begin / _update / _read against the NumPy comparator (solid_ref.py) after EVERY update: info ==, stamps ==,
finite doubles equal as int64 views, non-finite ones by class.

States and temperatures are uploaded, so every transition is under the test's control: upload A, begin, upload B, update,
...  solid_ref.sequence fills, empties and re-species a share of the voxels per update and makes the corners, edge mid points
and face centres of the lattice solidify, clear and solidify again.  The sizes cross the kernel's edges: a pair of k (odd L),
a row of pitchT doubles (L not a multiple of 8), a wave of 64 pairs, a pass of 256 and a block of 1024 pairs."""
import functools

import numpy as np
import pytest

import solid_ref as SR

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 5, 8, 9, 16, 17, 31, 33, 64, 65, 129)
STAMPS = (0, 20, 4000000000)                  # the last one does not fit 32 bits
DTS = (1e-6, 3e-6, 0.5)
INV_DX = 2.0e5


def _uniform_T(L, seed):
    return np.random.RandomState(seed).uniform(2900.0, 3700.0, (L, L, L))


@functools.lru_cache(maxsize=None)
def _sequence(L, uniform):
    seq = SR.sequence(L, 11 + L, T=_uniform_T if uniform else SR.grid_T)
    for st, T in seq:
        st.setflags(write=False)
        T.setflags(write=False)
    return seq


def _engine(L, state, T):
    import cetkmc
    e = cetkmc.Engine(L)
    z = np.zeros((L, L, L))
    e.upload(state, z, z, T, np.zeros((L, L, L), np.int64))
    return e


def _compare(e, ref, info, want, tag):
    assert info == want, (tag, info, want)
    assert SR.same_map(e.solid_read(), ref.map()) == [], tag


@pytest.mark.parametrize("L", SIZES)
def test_sequence(L):
    seq = _sequence(L, L <= 33)
    e = _engine(L, *seq[0])
    try:
        e.solid_begin()
        ref = SR.SolidRef(*seq[0])
        _compare(e, ref, dict(n_new=0, n_cleared=0, n_recorded=0), dict(n_new=0, n_cleared=0, n_recorded=0), (L, "begin"))
        seen = set()
        for u, (st, T) in enumerate(seq[1:]):
            e.upload(state=st, T=T)
            info = e.solid_update(STAMPS[u], DTS[u], INV_DX)
            want = ref.update(st, T, STAMPS[u], INV_DX, DTS[u])
            print(f"L={L} update {u}: {want}")
            _compare(e, ref, info, want, (L, u))
            seen |= {k for k in ("n_new", "n_cleared") if want[k]}
        assert seen == {"n_new", "n_cleared"}
        sp = SR.special_voxels(L)
        assert all(ref.stamp[v] == STAMPS[2] for v in sp)      # every face, edge and corner: solid, cleared, solid again
        d = e.download()                                       # the updates wrote no lattice field
        assert np.array_equal(d["state"], seq[-1][0]) and np.array_equal(d["T"], seq[-1][1])
        # an update without a change: nothing new, nothing cleared, the map stands; then a second begin resets it
        info = e.solid_update(7, 1.0, INV_DX)
        _compare(e, ref, info, ref.update(seq[-1][0], seq[-1][1], 7, INV_DX, 1.0), (L, "idle"))
        assert info["n_new"] == 0 and info["n_cleared"] == 0 and (info["n_recorded"] > 0 or L == 1)
        e.solid_begin()
        ref.begin(*seq[-1])
        assert SR.same_map(e.solid_read(), ref.map()) == []
        e.upload(state=seq[1][0], T=seq[1][1])
        _compare(e, ref, e.solid_update(1, 2.0, 1.0), ref.update(seq[1][0], seq[1][1], 1, 1.0, 2.0), (L, "after the second begin"))
        e.solid_end()
        with pytest.raises(RuntimeError, match="needs a map"):
            e.solid_read()
    finally:
        e.close()


@pytest.mark.parametrize("L", [2, 9, 33])
def test_non_finite_temperatures(L):
    """NaN and both infinities on new voxels, on their neighbours and in the snapshot: stored as they come"""
    seq = _sequence(L, True)
    bad = (np.nan, np.inf, -np.inf)
    rs = np.random.RandomState(L)
    Ts = []
    for u, (st, T) in enumerate(seq):
        T = T.copy()
        at = rs.randint(0, L, (max(6, L ** 3 // 8), 3))
        for q, v in enumerate(at):
            T[tuple(v)] = bad[(q + u) % 3]
        Ts.append(T)
    e = _engine(L, seq[0][0], Ts[0])
    try:
        e.solid_begin()
        ref = SR.SolidRef(seq[0][0], Ts[0])
        classes = (np.isnan, np.isposinf, np.isneginf)
        hit = {k: [False] * 3 for k in SR.MAP_FIELDS}
        for u in range(1, len(seq)):
            e.upload(state=seq[u][0], T=Ts[u])
            _compare(e, ref, e.solid_update(u, DTS[u - 1], INV_DX), ref.update(seq[u][0], Ts[u], u, INV_DX, DTS[u - 1]), (L, u))
            m = ref.map()
            rec = m["stamp"] >= 0
            for k in SR.MAP_FIELDS:
                hit[k] = [h or bool(c(m[k][rec]).any()) for h, c in zip(hit[k], classes)]
        assert L == 2 or all(all(h) for h in hit.values()), hit
    finally:
        e.close()


def test_refusals():
    import cetkmc
    L = 8
    st, T = _sequence(L, False)[0]

    def refused(e, call, text):
        assert call() != 0
        assert text in e.error(), e.error()

    e = cetkmc.Engine(L, n_slabs=2)
    try:
        z = np.zeros((L, L, L))
        e.upload(st, z, z, T, np.zeros((L, L, L), np.int64))
        refused(e, lambda: e.lib.cetkmc_solid_begin(e.h), "one slab")
        refused(e, lambda: e.lib.cetkmc_solid_update(e.h, 0, 1.0, 1.0, None), "one slab")
        refused(e, lambda: e.lib.cetkmc_solid_read(e.h, None, None, None, None), "one slab")
    finally:
        e.close()
    e = _engine(L, st, T)
    try:
        for call in (lambda: e.lib.cetkmc_solid_update(e.h, 0, 1.0, 1.0, None), lambda: e.lib.cetkmc_solid_read(e.h, None, None, None, None),
                     lambda: e.lib.cetkmc_solid_end(e.h)):
            refused(e, call, "needs a map")
        e.solid_begin()
        ref = SR.SolidRef(st, T)
        st1, T1 = _sequence(L, False)[1]
        e.upload(state=st1, T=T1)
        launches = e.counters()
        for stamp, inv_dx, dt, text in ((-1, 1.0, 1.0, "negative"), (0, 1.0, 0.0, "dt"), (0, 1.0, -1.0, "dt"), (0, 1.0, np.nan, "dt"),
                                        (0, 1.0, np.inf, "dt"), (0, np.nan, 1.0, "inv_dx"), (0, -np.inf, 1.0, "inv_dx")):
            refused(e, lambda: e.lib.cetkmc_solid_update(e.h, stamp, inv_dx, dt, None), text)
        refused(e, lambda: e.lib.cetkmc_ensemble_solid_begin(e.h), "not an ensemble handle")
        refused(e, lambda: e.lib.cetkmc_ensemble_solid_update(e.h, 0, 1.0, 1.0, None), "not an ensemble handle")
        refused(e, lambda: e.lib.cetkmc_ensemble_solid_end(e.h), "not an ensemble handle")
        assert e.counters()["bytes_d2h"] == launches["bytes_d2h"]
        assert SR.same_map(e.solid_read(), ref.map()) == []            # the refused updates changed nothing
        _compare(e, ref, e.solid_update(5, 1.0, 1.0), ref.update(st1, T1, 5, 1.0, 1.0), "after the refusals")
        d2h = e.counters()["bytes_d2h"]
        e.solid_read()
        assert e.counters()["bytes_d2h"] - d2h == L ** 3 * 48
        d2h = e.counters()["bytes_d2h"]
        stamp = np.zeros((L, L, L), np.int64)
        assert e.lib.cetkmc_solid_read(e.h, stamp.ctypes.data, None, None, None) == 0 and np.array_equal(stamp, ref.stamp)
        assert e.counters()["bytes_d2h"] - d2h == L ** 3 * 8
    finally:
        e.close()
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.0)] * 2)
    try:
        r1 = ens.replica(1)
        refused(r1, lambda: ens.lib.cetkmc_solid_begin(r1.h), "single-lattice handle")
        refused(r1, lambda: ens.lib.cetkmc_solid_begin(ens.h), "single-lattice handle")
        refused(r1, lambda: ens.lib.cetkmc_ensemble_solid_update(ens.h, 0, 1.0, 1.0, None), "cetkmc_ensemble_solid_begin")
        refused(r1, lambda: ens.lib.cetkmc_ensemble_solid_begin(r1.h), "not an ensemble handle")
        refused(r1, lambda: ens.lib.cetkmc_solid_read(r1.h, None, None, None, None), "needs a map")
    finally:
        ens.close()
