"""The comparator of the beam tables (tests/beam_ref.py) against the comparators it is built on, the
product's table builders (thermal_solver.scan_path / beam_table) against their definitions, and what the inputs of the GPU tests
(tests/beam_cases.py) exercise.  No GPU, no engine."""
import math

import numpy as np
import pytest

import beam_cases as bm
import beam_ref
import implicit_cases as ic
import implicit_ref
import thermal_solver
from oracle import oracle


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _lattice(L, signed_zero=False):
    lat, _, _, _ = ic.direct_lattice(L)
    if signed_zero:
        lat.T = lat.T.copy()
        lat.T[0, 0, 0], lat.T[L - 1, L - 2, 1], lat.T[L - 1, 0, 0] = -0.0, -0.0, -0.0
    return lat


# ---- the comparator --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("L", [1, 2, 5, 17])
def test_depth_one_is_the_implicit_update_from_the_product_plane(L, n):
    """D = 1, fi = [1.0]: every bit of implicit_ref.update fed q[j][k] = (amp * 1.0) * (gj[j] * gk[k]), -0.0 voxels in the
    input (inside and outside the footprint: the zero term turns them into +0.0 in both)"""
    t = bm.direct_table(L, 1)
    assert t["fi"].tolist() == [1.0]
    a, b = _lattice(L, signed_zero=L > 1), _lattice(L, signed_zero=L > 1)
    for u in (bm.U0, bm.U0 + 1, bm.U0 + 2):
        beam_ref.update(a, n, bm.DT, t, u, use_latent=True, scrub=False)
        implicit_ref.update(b, n, bm.DT, 2, beam_ref.product_plane(t, u - bm.U0), use_latent=True, scrub=False)
        assert np.array_equal(_bits(a.T), _bits(b.T)), (L, n, u)
        assert np.array_equal(a.prev_state, b.prev_state)


def test_an_off_row_is_the_sourceless_update():
    L = 9
    t = bm.direct_table(L, 2)
    assert t["amp"][2] == 0.0
    a, b = _lattice(L), _lattice(L)
    beam_ref.update(a, 1, bm.DT, t, bm.U0 + 2)
    implicit_ref.update(b, 1, bm.DT, 2, np.zeros((L, L)))
    assert np.array_equal(_bits(a.T), _bits(b.T))


@pytest.mark.parametrize("D", [1, 2, 24])
def test_zeroing_rows_outside_the_footprint_changes_no_bit(D):
    """a row (plane, j) with amp * fi[d] == 0 or gj[j] == 0 gets the term dt * (0.0 + latent_coef * 0.0): skipping its source
    arithmetic (what the kernel's ballot does) is the definition"""
    L = 24
    t = bm.direct_table(L, D)
    lat = _lattice(L)
    need = beam_ref.footprint_rows(t, L, 0)
    assert need.any() and not need[L - D:].all()
    qv = beam_ref.source(t, L, 0)
    assert not qv[~need].any()                        # nothing outside the footprint rows
    P = lat.params
    b_full = beam_ref.rhs(lat, bm.DT, t, 0, latent=False, scrub=False)
    zero_term = np.float64(bm.DT) * (np.float64(0.0) + np.float64(P.latent_coef) * np.float64(0.0))
    b_skip = np.where(need[:, :, None], b_full, lat.T + zero_term)
    assert np.array_equal(_bits(b_full), _bits(b_skip))


@pytest.mark.parametrize("D", [1, 3])
def test_heat_conservation_of_an_adiabatic_update(D):
    """adiabatic, far from the clip, no latent heat: sum(T_new - T_old) == dt * sum(qterm) within 1e-9 relative"""
    L = 24
    rs = np.random.RandomState(5)
    z = np.zeros((L, L, L), np.int64)
    lat = oracle.Lattice(z, z.astype(float), z.astype(float), rs.uniform(3300.0, 3500.0, (L, L, L)), z, impurity_c=0.1)
    t = bm.direct_table(L, D)
    T0 = lat.T.copy()
    beam_ref.update(lat, 1, bm.DT, t, bm.U0, use_latent=False, scrub=False)
    assert lat.T.min() > lat.params.T_clip_lo and lat.T.max() < lat.params.T_clip_hi
    want = bm.DT * math.fsum(beam_ref.qterm_of(lat, t, 0).ravel())
    got = math.fsum((lat.T - T0).ravel())
    assert want > 0 and abs(got - want) <= 1e-9 * want, (got, want)


# ---- the tables ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,pen", [(1, None), (2, None), (8, None), (8, 10e-6), (32, 25e-6)])
def test_depth_profile_sums_to_one(D, pen):
    t = thermal_solver.beam_table(40, thermal_solver.scan_path(40, "diagonal", 1.0), 0, 1, 10.0, depth=D, penetration=pen)
    s = math.fsum(t["fi"])
    assert t["fi"].size == D and abs(s - 1.0) <= 4 * np.spacing(1.0), s
    if pen is not None:
        assert np.all(np.diff(t["fi"]) < 0)
    beam_ref.check(t, 40)


@pytest.mark.parametrize("radius_vox", [1.5, 2.5, 10.0])
def test_absorbed_power_of_a_table_row(radius_vox):
    """amp dx^3 sum(gj) sum(gk) = power * absorptivity * erf(cutoff)^2 within 1e-4 (the rule's error for a Gaussian)"""
    L, dx = 96, oracle.VOXEL_SIZE
    path = lambda u: (47.3, 48.6, True)
    t = thermal_solver.beam_table(L, path, 0, 1, 7.0, beam_radius=radius_vox * dx, absorptivity=0.35, cutoff=3.0)
    got = t["amp"][0] * dx ** 3 * math.fsum(t["gj"][0]) * math.fsum(t["gk"][0])
    want = 7.0 * 0.35 * math.erf(3.0) ** 2
    assert abs(got - want) <= 1e-4 * want, (got, want)
    assert (t["gj"][0] == 0.0).sum() == L - np.count_nonzero(np.abs(np.arange(L) - 47.3) <= 3.0 * radius_vox)


@pytest.mark.parametrize("radius_vox,c", [(10.0, 20.3), (1.5, 20.3), (0.4, 7.0)])
def test_depth_one_without_cutoff_against_laser_source_plane(radius_vox, c):
    """per voxel within (4 a + 8) 2^-52 relative, a the voxel's exponent argument: exp amplifies the rounding of its argument
    by the argument, and the two forms round r^2 / r_b^2 differently"""
    L, dx = 32, oracle.VOXEL_SIZE
    t = thermal_solver.beam_table(L, lambda u: (c, c, True), 0, 1, 60.0, beam_radius=radius_vox * dx, cutoff=np.inf)
    got = beam_ref.product_plane(t, 0)
    want = thermal_solver.laser_source_plane(L, (0, c), 60.0, beam_radius=radius_vox * dx)
    ax = np.arange(L) - c
    a = (ax[:, None] ** 2 + ax[None, :] ** 2) / radius_vox ** 2
    ok = want > 0                      # (both underflow to 0 together far out)
    assert np.array_equal(got == 0, want == 0) or np.all(a[(got == 0) != (want == 0)] > 700)
    rel = np.abs(got[ok] - want[ok]) / want[ok]
    assert np.all(rel <= (4 * a[ok] + 8) * 2.0 ** -52), float((rel / ((4 * a[ok] + 8) * 2.0 ** -52)).max())


def test_scan_path_by_hand():
    L = 12
    p = thermal_solver.scan_path(L, "diagonal", 1.5, start=2.0)
    assert [p(u) for u in (0, 1, 4)] == [(2.0, 2.0, True), (3.5, 3.5, True), (8.0, 8.0, True)]
    # margin 1: tracks from k = 1 to k = 10, length 9, speed 2.5: n_t = 4 updates at k = 1, 3.5, 6, 8.5
    p = thermal_solver.scan_path(L, "line", 2.5, margin=1.0)
    assert [p(u) for u in range(5)] == [(5.5, 1.0, True), (5.5, 3.5, True), (5.5, 6.0, True), (5.5, 8.5, True), (5.5, 1.0, False)]
    p = thermal_solver.scan_path(L, "line", 2.5, start=3.0, margin=1.0)
    assert p(2) == (3.0, 6.0, True)
    p = thermal_solver.scan_path(L, "raster", 2.5, hatch=4.0, margin=1.0)
    assert [p(u) for u in (0, 3, 4, 7, 8, 11)] == [(1.0, 1.0, True), (1.0, 8.5, True), (5.0, 1.0, True), (5.0, 8.5, True),
                                                   (9.0, 1.0, True), (9.0, 8.5, True)]
    assert p(12) == (13.0, 1.0, False)                      # the fourth track lies beyond L - 1 - margin = 10: off
    p = thermal_solver.scan_path(L, "serpentine", 2.5, hatch=4.0, start=2.0, margin=1.0)
    assert [p(u) for u in (0, 3, 4, 5, 7, 8)] == [(2.0, 1.0, True), (2.0, 8.5, True), (6.0, 10.0, True), (6.0, 7.5, True),
                                                  (6.0, 2.5, True), (10.0, 1.0, True)]
    assert p(12)[2] is False
    for bad in (dict(pattern="zigzag", speed=1.0), dict(pattern="raster", speed=1.0), dict(pattern="line", speed=0.0),
                dict(pattern="line", speed=1.0, margin=6.0)):
        with pytest.raises(ValueError):
            thermal_solver.scan_path(L, **bad)


@pytest.mark.parametrize("pattern", thermal_solver.SCAN_PATTERNS)
def test_adjacent_batches_concatenate_and_the_last_track_switches_off(pattern):
    L = 12
    p = thermal_solver.scan_path(L, pattern, 2.5, hatch=4.0, margin=1.0)
    kw = dict(power=3.0, beam_radius=bm.RADIUS, depth=2)
    a, b, c = (thermal_solver.beam_table(L, p, u0, n, **kw) for u0, n in ((0, 7), (7, 8), (0, 15)))
    for f in ("amp", "gj", "gk"):
        assert np.array_equal(_bits(np.concatenate([a[f], b[f]])), _bits(c[f])), f
    assert np.array_equal(a["fi"], c["fi"]) and (a["u0"], b["u0"]) == (0, 7)
    if pattern != "diagonal":
        assert c["amp"][0] > 0 and c["amp"][-1] == 0.0


def test_table_refusals_of_the_builders():
    p = thermal_solver.scan_path(8, "diagonal", 1.0)
    for kw in (dict(n_u=0), dict(depth=0), dict(depth=9), dict(beam_radius=0.0), dict(depth=2, penetration=-1.0)):
        with pytest.raises(ValueError):
            thermal_solver.beam_table(8, p, 0, **{"n_u": 1, "power": 1.0, **kw})
    t = thermal_solver.beam_table(8, p, 0, 2, 1.0)
    for f, v in (("amp", -1.0), ("gj", np.nan), ("gk", np.inf), ("fi", -0.5)):
        bad = {k: np.array(x, copy=True) if isinstance(x, np.ndarray) else x for k, x in t.items()}
        bad[f].flat[0] = v
        with pytest.raises(ValueError):
            beam_ref.check(bad, 8)
    with pytest.raises(ValueError):
        beam_ref.row_of(t, 2)


# ---- the stepper -----------------------------------------------------------------------------------------------------
def test_stepper_cut_into_two_calls_equals_one_call():
    case = dict(bm.STEPPING["L24_nolatent_rng1_incr_n1_D4"], use_latent=True)
    one = bm.run_case(dict(case, batches=(47,)))
    two = bm.run_case(dict(case, batches=(47,)))
    full = bm.calls_of(dict(case, batches=(47,)))[0]
    s0, n, up, ud, unp, _ = full
    lat = oracle.Lattice(*one["lat0"], impurity_c=0.1)
    st = beam_ref.Stepper(lat, bm.table_of(dict(case, batches=(47,))), case["n_sub"])
    r1 = st.run_steps(0, 27, case["defect_fraction"], up[:27], ud[:27], unp, rng_mode=1, seed=case["seed"], thermal_mode=2, use_latent=True)
    r2 = st.run_steps(27, 20, case["defect_fraction"], up[27:], ud[27:], unp[r1["np_used"]:], rng_mode=1, seed=case["seed"], thermal_mode=2,
                      use_latent=True)
    assert (r1["done"], r2["done"]) == (27, 20) and st.beam_updates == 3
    assert np.array_equal(_bits(np.concatenate([r1["totals"], r2["totals"]])), _bits(one["results"][0]["totals"]))
    for got, want in zip((lat.state, lat.theta, lat.phi, lat.T, lat.prev_state), one["fields"][0]):
        assert got.tobytes() == want.tobytes()
    assert two["fields"][0][3].tobytes() == one["fields"][0][3].tobytes()        # and the run is repeatable


# ---- what the GPU tests' inputs exercise -----------------------------------------------------------------------------
@pytest.mark.parametrize("L,D,n,latent", [c for c in bm.DIRECT if c[0] <= 65 or c[2:] == (1, True)])       # (129: one case per depth)
def test_direct_inputs(L, D, n, latent):
    T, stats = bm.direct_reference(L, D, n, latent)
    t = bm.direct_table(L, D)
    assert np.isfinite(T).all() and stats["updates"] == 2 and stats["source"] == 2
    assert stats["heated_max"] < ic.CLIP_HI, stats["heated_max"]              # the heated voxels stay off T_clip_hi
    assert (stats["latent"] > 0) == latent
    for x in (0, 1):
        need = beam_ref.footprint_rows(t, L, x)
        if D > 1:       # a source row is non-zero in at least two depth planes
            assert (need.sum(axis=0) >= 2).any() and np.count_nonzero(beam_ref.source(t, L, x).any(axis=(1, 2))) == D
        if L > 9:       # (a lattice up to 9 wide lies inside the 9 non-zero factors) rows of the footprint's planes with gj == 0
            assert not need[L - D:].all()
    assert t["amp"][2] == 0.0


@pytest.mark.parametrize("L", [9, 65])
def test_nonfinite_input_in_the_footprint(L):
    T, stats = bm.nonfinite_reference(L, 2, 3)
    assert (stats["nan_before"], stats["inf_before"]) == (1, 1) and np.isfinite(T).all()


# (the L = 136 case takes the comparator 20 s: the GPU test that runs it checks its update count and its deferred steps)
@pytest.mark.parametrize("name", [n for n in bm.STEPPING if not n.startswith("L136")] + list(bm.ENSEMBLE))
def test_stepping_inputs(name):
    case = {**bm.STEPPING, **bm.ENSEMBLE}[name]
    run = bm.stepped(name)
    st = run["stepper"]
    t = st.table
    assert st.beam_updates >= 2 and 2 <= st.stats["source"] <= st.beam_updates        # (the scan's third track lies off the lattice)
    assert st.stats["nan_before"] >= 1 and st.stats["inf_before"] >= 1          # a NaN and a +inf stand in front of an update
    assert (st.stats["latent"] > 0) == case["use_latent"]
    assert t["u0"] == case["step0"] // 20
    assert len({tuple(r) for r in np.round(t["gj"], 12)}) >= 2                  # the second track begins inside the run
    if case["remelt"]:
        assert st.info["n_melted"] > 0
    if case["bc"] is not None:
        assert st.bc_updates == st.beam_updates
    need = beam_ref.footprint_rows(t, case["L"], 0)
    assert need.any() and not need[case["L"] - case["depth"]:].all()
    # the heated voxels stay off T_clip_hi (the planted hot block is elsewhere: its voxels may sit there)
    T = run["fields"][-1][3]
    hot = beam_ref.source(t, case["L"], int(np.flatnonzero(t["amp"])[-1])) != 0.0
    assert T[hot].max() < ic.CLIP_HI
    assert all(np.isfinite(r["totals"]).all() for r in run["results"])
