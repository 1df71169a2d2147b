"""Thermal boundary conditions without a device: the library's host routine cetkmc_implicit_coeffs_bc
against the comparator's coefficients bit for bit and its refusals; the comparator (tests/boundary_ref.py) against a dense
matrix, the maximum principle, the heat balance, L = 1, the adiabatic case against tests/implicit_ref.py, the Stepper's update
ordinal across calls; the product's boundary builders; and every input of the GPU files (tests/boundary_cases.py) for what it is
meant to exercise."""
import numpy as np
import pytest

import boundary_cases as bc
import boundary_ref as br
import implicit_cases as ic
import implicit_ref

BETAS = ((0.37, 0.0), (0.0, 1.0), (1.0, 2.5))


def _r(oracle_mod, dt):
    P = oracle_mod.make_params(0.1)
    return (P.alpha * dt) * P.inv_dx2


@pytest.mark.parametrize("L", [1, 2, 3, 7, 256])
def test_library_coefficients(oracle_mod, L):
    """both beta 0: cetkmc_implicit_coeffs bit for bit; the three beta pairs: the comparator's, for the r of dt, of dt / 17, and 0"""
    import cetkmc
    for r in (_r(oracle_mod, 1e-6), _r(oracle_mod, 1e-6 / 17), 0.0):
        inv, p = cetkmc.implicit_coeffs_bc(L, r, 0.0, 0.0)
        winv, wp = cetkmc.implicit_coeffs(L, r)
        assert inv.tobytes() == winv.tobytes() and p.tobytes() == wp.tobytes(), (L, r)
        rinv, rp = br.coeffs(L, r)
        assert inv.tobytes() == rinv.tobytes() and p.tobytes() == rp.tobytes(), (L, r)
        for lo, hi in BETAS:
            inv, p = cetkmc.implicit_coeffs_bc(L, r, lo, hi)
            winv, wp = br.coeffs(L, r, lo, hi)
            assert inv.tobytes() == winv.tobytes() and p.tobytes() == wp.tobytes(), (L, r, lo, hi)


def test_library_coefficients_refusals():
    import cetkmc
    for L, r, lo, hi, word in ((0, 1.0, 0, 0, "L must be"), (-3, 1.0, 0, 0, "L must be"), (4, np.nan, 0, 0, "r is not finite"),
                               (4, np.inf, 0, 0, "r is not finite"), (4, -1e-300, 0, 0, "r must be >= 0"), (4, 1.0, -1e-300, 0, "beta must be >= 0"),
                               (4, 1.0, 0, -2.0, "beta must be >= 0"), (4, 1.0, np.nan, 0, "beta is not finite"), (4, 1.0, 0, np.inf, "beta is not finite")):
        with pytest.raises(ValueError, match="cetkmc_implicit_coeffs_bc") as err:
            cetkmc.implicit_coeffs_bc(L, r, lo, hi)
        assert word in str(err.value)
        with pytest.raises(ValueError):
            br.coeffs(L, r, lo, hi)


def _dense(L, r, lo, hi):
    D = -2.0 * np.eye(L) + np.eye(L, k=1) + np.eye(L, k=-1)
    D[0, 0] = -(1.0 + lo)
    D[L - 1, L - 1] = -(1.0 + hi) if L > 1 else -(lo + hi)
    return np.eye(L) - r * D


def test_solve_against_a_dense_matrix(oracle_mod):
    """L = 7, beta = (0.37, 1), T_ext = (500, 4000): the residual of (I - r D_bc) x = b + c stays below 1e-10 K along each axis
    (the bound of tests/test_implicit_ref_host.py's dense test)"""
    L, lo, hi, Tlo, Thi = 7, 0.37, 1.0, 500.0, 4000.0
    r = _r(oracle_mod, 1e-6)
    A = _dense(L, r, lo, hi)
    b = np.random.RandomState(0).uniform(0.0, 4100.0, (L, L, L))
    inv, p = br.coeffs(L, r, lo, hi)
    c_lo, c_hi = (r * lo) * Tlo, (r * hi) * Thi
    worst = 0.0
    for axis in range(3):
        x = br.solve(b, axis, r, inv, p, c_lo, c_hi)
        rhs = np.moveaxis(b, axis, 0).copy()
        rhs[0] += c_lo
        rhs[L - 1] += c_hi
        res = np.tensordot(A, np.moveaxis(x, axis, 0), axes=1) - rhs
        worst = max(worst, float(np.abs(res).max()))
    print("largest residual", worst)
    assert worst <= 1e-10


@pytest.mark.parametrize("L", [1, 2, 7, 33])
def test_maximum_principle_and_heat_balance(oracle_mod, L):
    """per solve: the result lies within the range of b and the active T_f; sum(x - b) == r * sum_f beta_f (T_f - x_face) within
    1e-9 relative (to the larger side's magnitude)"""
    rs = np.random.RandomState(L)
    for r in (_r(oracle_mod, 1e-6), _r(oracle_mod, 1e-6 / 17)):
        for (lo, hi), (Tlo, Thi) in zip(BETAS + ((0.0, 0.0),), ((500.0, 0.0), (0.0, 4000.0), (5000.0, 100.0), (9e9, -9e9))):
            b = rs.uniform(2800.0, 4064.5, (L, 5, 3))
            inv, p = br.coeffs(L, r, lo, hi)
            x = br.solve(b, 0, r, inv, p, (r * lo) * Tlo if lo else None, (r * hi) * Thi if hi else None)
            act = [T for beta, T in ((lo, Tlo), (hi, Thi)) if beta]
            lo_b, hi_b = min([b.min()] + act), max([b.max()] + act)
            assert x.min() >= lo_b - 1e-9 and x.max() <= hi_b + 1e-9, (L, lo, hi)
            lhs = float((x - b).sum())
            rhs = float(r * (lo * (Tlo - x[0]).sum() + hi * (Thi - x[L - 1]).sum()))
            print(L, lo, hi, lhs, rhs)
            if act:
                assert abs(lhs - rhs) <= 1e-9 * max(abs(lhs), abs(rhs)), (L, lo, hi, lhs, rhs)
            else:       # insulated: both sides vanish but for rounding, a few ulp of each of the summed values
                assert rhs == 0.0 and abs(lhs) <= 1e-12 * float(np.abs(b).sum()), (L, lhs)


def test_one_voxel(oracle_mod):
    """L = 1: the diagonal is 1 + r (beta_lo + beta_hi) per axis and the right side ((b + c_lo) + c_hi)"""
    z = np.zeros((1, 1, 1))
    lat = oracle_mod.Lattice(z.astype(np.int64), z, z, z + 3333.0, impurity_c=0.1)
    r = _r(oracle_mod, 1e-6)
    b = br.boundary(beta=(0.37, 1.0, 0.0, 0.0, 0.5, 0.0), T_ext=(3000.0, 3500.0, 9e9, 9e9, 3100.0, 9e9))
    br.update(lat, 1, 1e-6, 1, bc=b)
    x = np.float64(3333.0)
    x = (x + (r * 0.5) * 3100.0) * (1.0 / (1.0 + r * (0.5 + 0.0)))                              # axis 2
    x = x * (1.0 / (1.0 + r * 0.0))                                                             # axis 1: adiabatic, the identity
    x = ((x + (r * 0.37) * 3000.0) + (r * 1.0) * 3500.0) * (1.0 / (1.0 + r * (0.37 + 1.0)))     # axis 0
    assert lat.T[0, 0, 0] == x and 3000.0 < x < 3500.0


def test_gradient_boundary_holds_the_ramp(oracle_mod):
    """L = 12, 50 updates at the default dt: within 1e-9 K of build_temperature_field's ramp with thermal_solver.gradient_boundary
    (1.0e-11 K measured; two decades left for other L); between insulated walls the first update alone moves it by more than
    1 K (99 K measured)"""
    import thermal_solver
    L = 12
    T0 = thermal_solver.build_temperature_field(L)
    z = np.zeros((L, L, L))
    g = bc.gradient(L)
    held, free = (oracle_mod.Lattice(z.astype(np.int64), z, z, T0, impurity_c=0.0) for _ in range(2))
    br.update(free, 1, 1e-6, 1, bc=None)
    print("adiabatic, one update:", np.abs(free.T - T0).max())
    assert np.abs(free.T - T0).max() > 1.0
    for u in range(50):
        br.update(held, 1, 1e-6, 1, bc=g, u=u)
    print("gradient boundary, 50 updates:", np.abs(held.T - T0).max())
    assert np.abs(held.T - T0).max() <= 1e-9


def test_product_boundary_builders():
    """beta = h * VOXEL_SIZE / K, ramp = -cooling_rate * dt on the fixed faces only, the face order, the refusals"""
    import thermal_solver as ts
    from constants import T_MELT, T_SUB, VOXEL_SIZE
    assert ts.FACES == br.FACES
    b = ts.thermal_boundary(bottom=("fixed", 2800.0), top=("convective", 2.0e6, 300.0), sides="adiabatic", cooling_rate=1e6, dt=2e-6)
    assert b["beta"] == [1.0, 2.0e6 * VOXEL_SIZE / 173.0, 0.0, 0.0, 0.0, 0.0]
    assert b["T_ext"] == [2800.0, 300.0, 0.0, 0.0, 0.0, 0.0]
    assert b["ramp"] == [-2.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    b = ts.thermal_boundary(sides=("convective", 1.73e8, 500.0))
    assert b["beta"] == [0.0, 0.0] + [1.73e8 * VOXEL_SIZE / 173.0] * 4 and b["T_ext"] == [0.0, 0.0] + [500.0] * 4 and b["ramp"] == [0.0] * 6
    assert ts.thermal_boundary() == dict(beta=[0.0] * 6, T_ext=[0.0] * 6, ramp=[0.0] * 6)
    g = ts.gradient_boundary(12, cooling_rate=1e6)
    slope = (T_MELT - T_SUB) / 11
    assert g["beta"] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0] and g["T_ext"][:2] == [T_SUB - slope, T_MELT + slope] and g["ramp"][:2] == [-1.0, -1.0]
    for bad in ("fixed", ("fixed",), ("convective", 1.0), ("radiative", 1.0, 2.0), 5):
        with pytest.raises(ValueError, match="thermal_boundary"):
            ts.thermal_boundary(top=bad)
    with pytest.raises(ValueError, match="implicit"):
        ts.update_temperature_cet(np.zeros((2, 2, 2)), None, boundary=b)            # refused before any device call
    with pytest.raises(ValueError, match="implicit"):
        ts.update_temperature(np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), np.zeros((2, 2, 2)), 1e-6, (0, 0), 1.0, boundary=b)


@pytest.mark.parametrize("L", [1, 3, 10])
@pytest.mark.parametrize("key", ["none", "zero"])
def test_every_beta_zero_is_the_adiabatic_comparator(oracle_mod, L, key):
    """bit for bit tests/implicit_ref.update, with -0.0 voxels in the input (an adiabatic face adds nothing, not even + 0.0)"""
    lat_a, _, _, q = ic.direct_lattice(L)
    lat_b, _, _, _ = ic.direct_lattice(L)
    for lat in (lat_a, lat_b):
        T = lat.T.copy()
        T[0, 0, 0] = -0.0
        T[L - 1, L - 1, L - 1] = -0.0
        lat.T = T
    lat_a.params.T_clip_lo = lat_b.params.T_clip_lo = -1.0          # the clip would turn -0.0 into T_clip_lo
    for mode in (1, 2):
        implicit_ref.update(lat_a, 2, 1e-6, mode, q)
        br.update(lat_b, 2, 1e-6, mode, q, bc=bc.BOUNDARIES[key], u=3)
        assert lat_a.T.tobytes() == lat_b.T.tobytes() and lat_a.prev_state.tobytes() == lat_b.prev_state.tobytes(), mode
    if L == 1:
        z = np.zeros((1, 1, 1))
        one = oracle_mod.Lattice(z.astype(np.int64), z, z, np.full((1, 1, 1), -0.0), impurity_c=0.1)
        one.params.T_clip_lo = -1.0
        br.update(one, 1, 1e-6, 1, bc=bc.BOUNDARIES[key])
        assert np.signbit(one.T[0, 0, 0])                   # -0.0 in, -0.0 out


def test_stepper_split_into_two_calls_equals_one_call(oracle_mod):
    """a non-zero ramp: the update of global step g uses u = g // 20 however the run is cut (rng_mode 2: no streams to cut)"""
    case = dict(bc.STEPPING["L40_cet_rng2_full_n3_ramp"], n_sub=1)
    one = bc.run_case(dict(case, batches=(46,)))
    two = bc.run_case(dict(case, batches=(27, 19)))
    for a, b in zip(one["fields"][-1], two["fields"][-1]):
        assert a.tobytes() == b.tobytes()
    assert one["stepper"].bc_updates == two["stepper"].bc_updates == 3
    flat = bc.run_case(dict(case, batches=(46,), bc=bc.gradient(case["L"])))
    assert np.abs(flat["fields"][-1][3] - one["fields"][-1][3]).max() > 1.0        # the ramp is felt


def _assert_faces_felt(T, T_adiabatic, boundary, tag):
    for f, sl in enumerate(bc.face_slices(T.shape[0])):
        if boundary["beta"][f] != 0.0:
            assert np.nanmax(np.abs(T[sl] - T_adiabatic[sl])) > 1.0, (tag, br.FACES[f])


@pytest.mark.parametrize("L", bc.SIZES)
def test_direct_inputs_hold_what_they_claim(oracle_mod, L):
    """the all-six boundary and every single face: at least one voxel of each active face differs by more than 1 K from the
    adiabatic result; voxels on both clip values after some step (L >= 5, as in tests/test_implicit_ref_host.py: smaller
    lattices have no room for the cold planes beside the beam); latent heat released and a non-zero source in laser mode; a NaN
    and infinities in front of step 1 of the non-finite set (L >= 3), none left"""
    for mode in (1, 2):
        free, _ = bc.direct_reference(L, 1, mode, "none")
        for key in ("all",) + (br.FACES if L == 9 else ()):
            T, st = bc.direct_reference(L, 1, mode, key)
            _assert_faces_felt(T, free, bc.BOUNDARIES[key], (L, mode, key))
            if L >= 5 and key == "all":
                assert st["on_clip_lo"] > 0 and st["on_clip_hi"] > 0, (L, mode, st)
            if mode == 2:
                assert st["latent"] > 0 and st["source"] == 2
    if L >= 3:
        T, st = bc.direct_reference(L, 3, 2, "all", nonfinite=True, updates=1)
        assert st["nan_before"] >= 1 and st["inf_before"] >= 2 and np.isfinite(T).all()


def _assert_run_holds(case, run, free, tag, steps=True):
    st = run["stepper"].stats
    assert st["updates"] >= 1 and st["substeps"] == st["updates"] * case["n_sub"], tag
    assert st["nan_before"] >= 1 and st["inf_before"] >= 1, (tag, st)
    assert st["on_clip_lo"] > 0 and st["on_clip_hi"] > 0, (tag, st)
    assert run["stepper"].bc_updates == st["updates"], tag
    if case["thermal_mode"] == 2:
        assert st["source"] == st["updates"], (tag, st)
        if case["use_latent"] and steps:
            assert st["latent"] > 0, (tag, st)
    if free is not None:
        _assert_faces_felt(run["fields"][0][3], free["fields"][0][3], bc._bc_of(case), tag)
    if steps:
        assert len(run["results"]) == len(run["calls"]) and all(r["status"] == 0 for r in run["results"]), tag
        assert st["updates"] >= 2, tag
        assert all(np.isfinite(r["totals"]).all() for r in run["results"]), tag


@pytest.mark.parametrize("name", list(bc.STEPPING))
def test_stepping_inputs_hold_what_they_claim(oracle_mod, name):
    case = bc.STEPPING[name]
    run = bc.stepped(name)
    _assert_run_holds(case, run, bc.stepped_adiabatic_first_call(name), name)
    if case["remelt"]:
        assert run["stepper"].info["n_melted"] > 0


@pytest.mark.parametrize("name,R", [("ens_L30_n1_bc", 3), ("ens_L33_n3_bc", 70)])
def test_ensemble_inputs_hold_what_they_claim(oracle_mod, name, R):
    case, runs = bc.replica_runs(name, R)
    seen = set()
    for r, (run, _) in enumerate(runs):
        if id(run) in seen:
            continue
        seen.add(id(run))
        _assert_run_holds(case, run, bc.stepped_adiabatic_first_call(name) if r == 2 else None, (name, r), steps=r != 0)
    cold = runs[0][0]
    assert cold["results"][0]["status"] == 1 and cold["results"][0]["done"] == 0 and cold["stepper"].stats["updates"] == 1
