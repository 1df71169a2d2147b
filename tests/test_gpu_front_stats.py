"""cetkmc_front_stats / cetkmc_ensemble_front_stats against the NumPy comparator (front_ref.py): every lattice size at which
the kernel takes another path, empty / full lattices, the melt bounding box, non-finite temperatures, determinism, the
stream ordering behind stepping work, ensembles (bits of a replica = bits of a single handle) and the refusals.

Bounds (derived, not tuned): integer fields and the bounding box exact; G_min / G_max equal to the comparator's per-voxel
values (every operation but the square root is correctly rounded on both sides; the definition grants the square root
1 ulp, and on the MI355X it agreed bit for bit in every case of this file, so the check is equality); each sum within
n_front * 2^-53 * fsum(|x|) of math.fsum -- the worst case of any summation order -- plus 1 ulp per term for G."""
import functools

import numpy as np
import pytest

from front_ref import check_stats, front_ref, front_ref_stats

pytestmark = pytest.mark.gpu

SHAPES = (1, 2, 3, 5, 33, 64, 65, 128, 129)


def _consts():
    import constants as K
    return float(K.T_MELT), float(K.T_SUB), 1.0 / K.VOXEL_SIZE


def _lattice(L, seed, hot=True):
    """~40 % occupancy with all five state codes (L >= 3), T = the substrate-to-melt ramp along i plus noise; with ``hot``
    the top planes reach past T_melt here and there."""
    T_melt, T_sub, _ = _consts()
    rs = np.random.RandomState(seed)
    state = np.where(rs.random_sample((L, L, L)) < 0.4, rs.randint(1, 5, (L, L, L)), 0).astype(np.int64)
    if L >= 3:
        state.reshape(-1)[rs.choice(L ** 3, 5, replace=False)] = np.arange(5)
    ramp = T_sub + ((T_melt if hot else T_melt - 200.0) - T_sub) * (np.arange(L) / max(L - 1, 1))
    T = ramp[:, None, None] + 25.0 * rs.standard_normal((L, L, L))
    return state, np.ascontiguousarray(T)


@functools.lru_cache(maxsize=None)
def _case(L):
    state, T = _lattice(L, 1000 + L)
    T_melt, _, inv_dx = _consts()
    ref = front_ref(state, T, T_melt, inv_dx)
    state.setflags(write=False)
    T.setflags(write=False)
    return state, T, ref, front_ref_stats(ref, T)


def _want(state, T):
    T_melt, _, inv_dx = _consts()
    ref = front_ref(state, T, T_melt, inv_dx)
    return ref, front_ref_stats(ref, T)


def _engine(L, state, T, **kw):
    import cetkmc
    e = cetkmc.Engine(L, **kw)
    z = np.zeros((L, L, L))
    e.upload(state, z, z, T, np.zeros((L, L, L), np.int64))
    return e


def _same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a) and set(a) == set(b)


@pytest.mark.parametrize("L", SHAPES)
def test_shapes(L):
    state, T, ref, want = _case(L)
    if L >= 5:
        assert want["n_front"] >= L * L and set(np.unique(state)) == {0, 1, 2, 3, 4}
        f = ref["front"]
        assert all(x.any() for x in (f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1])), "front voxels on all six faces"
        assert want["n_melt"] > 0
    if L == 1:
        assert want["n_front"] == 0
    e = _engine(L, state, T)
    try:
        got, again = e.front_stats(), e.front_stats()
    finally:
        e.close()
    check_stats(got, want, f"L={L}")
    print(f"L={L}: n_front {want['n_front']} n_melt {want['n_melt']}")
    assert _same_bits(got, again)


@pytest.mark.parametrize("L", (5, 33))
def test_empty_and_full(L):
    _, T, _, _ = _case(L)
    for fill in (0, 2):
        state = np.full((L, L, L), fill, np.int64)
        e = _engine(L, state, T)
        try:
            got = e.front_stats()
        finally:
            e.close()
        assert got["n_front"] == 0 and got["n_skipped"] == 0 and got["G_min"] == 0.0 and got["G_max"] == 0.0
        assert got["G_sum"] == 0.0 and got["T_sum"] == 0.0 and list(got["pos_sum"]) == [0, 0, 0]
        check_stats(got, _want(state, T)[1], f"L={L} fill={fill}")


def test_melt_box_and_empty_sentinel():
    L = 33
    T_melt = _consts()[0]
    state, T = _lattice(L, 7, hot=False)
    ref, want = _want(state, T)
    assert want["n_melt"] == 0 and list(want["melt_bbox"]) == [L, L, L, -1, -1, -1]
    e = _engine(L, state, T)
    try:
        got = e.front_stats()
        check_stats(got, want, "no melt")
        assert list(got["melt_bbox"]) == [L, L, L, -1, -1, -1]
        T = T.copy()
        T[L - 4:, 0:6, 10:21] = T_melt + 50.0            # touches plane L-1 and the j = 0 face
        T[L - 1, 0, 10] = T_melt                          # >= : exactly T_melt is a melt voxel
        e.upload(T=T)
        got = e.front_stats()
    finally:
        e.close()
    assert list(got["melt_bbox"]) == [L - 4, 0, 10, L - 1, 5, 20] and got["n_melt"] == 4 * 6 * 11
    check_stats(got, _want(state, T)[1], "hot box")


def test_non_finite():
    L = 33
    state, T0, ref0, _ = _case(L)
    T = T0.copy()
    inner = np.zeros((L, L, L), bool)
    inner[2:-2, 2:-2, 2:-2] = True
    fr = np.argwhere(ref0["front"] & inner)
    nf = np.argwhere(~ref0["front"] & ~ref0["skipped"] & inner)
    vals = (np.nan, np.inf, -np.inf)
    for q, v in enumerate(vals):
        a = tuple(fr[40 * q])                             # at a front voxel
        b = tuple(fr[40 * q + 500] + (1, 0, 0))           # at the i+1 neighbour of a front voxel
        c = tuple(nf[97 * q + 11])                        # at a voxel that is no front voxel
        for p in (a, b, c):
            T[p] = v
    ref, want = _want(state, T)
    assert want["n_skipped"] >= 3
    n_inf = int(np.isposinf(T).sum())
    assert n_inf == 3 and ref["melt"][np.isposinf(T)].all() and not ref["melt"][np.isnan(T)].any()
    e = _engine(L, state, T)
    try:
        got = e.front_stats()
    finally:
        e.close()
    print(f"non-finite: n_skipped {want['n_skipped']} n_front {want['n_front']} n_melt {want['n_melt']}")
    check_stats(got, want, "non-finite")


@pytest.mark.parametrize("thermal_mode", (1, 2))
def test_after_stepping(thermal_mode):
    """40 batched steps with two temperature updates (the T buffer pair flips twice... and once more below), then the
    statistics of what a download shows: the call is ordered behind the stepping work and reads the current T buffer."""
    import cetkmc
    import lattice_init
    from thermal_solver import laser_scan_planes
    L = 33
    np.random.seed(11)
    state, theta, phi, T, _ = lattice_init.initialize_lattice(lattice_size=L, n_seeds=6, impurity_c=0.1)
    e = cetkmc.Engine(L, impurity_c=0.1)
    try:
        e.upload(state, theta, phi, T, np.zeros((L, L, L), np.int64))
        before = e.front_stats()
        laser = dict(power=200.0, start=10.0, speed=2.0)
        for step0, n in ((0, 40), (40, 1)):               # the second call holds the third update: the other parity
            q = laser_scan_planes(L, laser, step0, n) if thermal_mode == 2 else None
            r = e.run_steps(step0, n, 0.0, None, None, None, rng_mode=2, seed=5, thermal_mode=thermal_mode, q_planes=q)
            assert r["done"] == n and r["status"] == 0
            got = e.front_stats()
            d = e.download()
            check_stats(got, _want(d["state"], d["T"])[1], f"thermal_mode={thermal_mode} after step {step0 + n}")
            assert not np.array_equal(d["T"], T)
        assert not _same_bits(before, got)
    finally:
        e.close()


def _frozen_lattice(L, seed):
    """No event is possible (defect voxels and empty ones only, plane L-1 full, every T within delta_T_c of T_melt): the
    replica terminates in its first step and is frozen -- yet it has a front and a melt pool."""
    T_melt = _consts()[0]
    rs = np.random.RandomState(seed)
    state = np.where(rs.random_sample((L, L, L)) < 0.5, 4, 0).astype(np.int64)
    state[L - 1] = 4
    return state, T_melt - 5.0 * rs.random_sample((L, L, L)) + 6.0 * (rs.random_sample((L, L, L)) < 0.1)


@pytest.mark.parametrize("R,L", [(1, 8), (3, 8), (70, 8), (1, 33), (3, 33), (70, 33), (4, 128)])
def test_ensembles(R, L):
    import cetkmc
    lat = [_lattice(L, 50 * L + r, hot=(r % 2 == 0)) for r in range(R)]
    fz = R // 2
    lat[fz] = _frozen_lattice(L, 99)
    params = [cetkmc.default_params(0.05 * (r % 4)) for r in range(R)]
    z, zi = np.zeros((L, L, L)), np.zeros((L, L, L), np.int64)
    ens = cetkmc.Ensemble(L, params)
    one = cetkmc.Engine(L)
    try:
        for r, (s, T) in enumerate(lat):
            ens.replica(r).upload(s, z, z, T, zi)
        res = ens.run(0, 2, 0.0, rng_mode=2, seeds=np.arange(R) + 3, thermal_mode=0)
        assert res["status"][fz] == 1 and res["done"][fz] == 0, "the frozen replica"
        assert all(res["status"][r] == 0 and res["done"][r] == 2 for r in range(R) if r != fz)
        got = ens.front_stats()
        assert all(v.shape[0] == R for v in got.values())
        again = ens.front_stats()
        assert _same_bits(got, again)
        for r in range(R):
            d = ens.replica(r).download()
            mine = {k: (v[r] if v[r].ndim else v[r].item()) for k, v in got.items()}
            want = _want(d["state"], d["T"])[1]
            check_stats(mine, want, f"R={R} L={L} replica {r}")
            if r == fz:
                assert want["n_front"] > 0 and want["n_melt"] > 0 and np.array_equal(d["state"], lat[fz][0])
            assert _same_bits(mine, ens.replica(r).front_stats()), r
            one.upload(d["state"], d["theta"], d["phi"], d["T"], zi)
            assert _same_bits(mine, one.front_stats()), r
        assert len({int(x) for x in got["n_front"]}) == R or R > 8       # the replicas do hold different lattices
    finally:
        one.close()
        ens.close()


def test_refusals():
    import cetkmc
    L = 8
    state, T = _lattice(L, 3)
    e = _engine(L, state, T, n_slabs=2)
    try:
        with pytest.raises(RuntimeError, match="one slab"):
            e.front_stats()
        assert e.error()
    finally:
        e.close()
    e = _engine(L, state, T)
    try:
        buf = np.zeros(1, dtype=cetkmc.engine.FRONT_DTYPE)
        rc = e.lib.cetkmc_ensemble_front_stats(e.h, 1.0, buf.ctypes.data)
        assert rc != 0 and "ensemble" in e.error()
        rc = e.lib.cetkmc_front_stats(e.h, 1.0, None)
        assert rc != 0 and e.error()
    finally:
        e.close()
