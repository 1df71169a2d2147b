"""The implicit scheme without a device: the library's host routine cetkmc_implicit_coeffs against the
comparator's coefficients bit for bit; the comparator (tests/implicit_ref.py) against a dense solve, at L = 1, and on the rough
field of the stability table; its chunked stepper's plumbing against the oracle's unbroken run; and every input of the GPU files
(tests/implicit_cases.py: direct, stepping and ensemble) for what it is meant to exercise."""
import numpy as np
import pytest

import implicit_cases as ic
import implicit_ref
import remelt_cases as rc
import substep_cases as sc
import substep_ref


def _r(oracle_mod, dt):
    P = oracle_mod.make_params(0.1)
    return (P.alpha * dt) * P.inv_dx2


@pytest.mark.parametrize("L", [1, 2, 3, 7, 256])
def test_library_coefficients_equal_the_comparators(oracle_mod, L):
    """r of the default dt, of dt / 17, and 0"""
    import cetkmc
    for r in (_r(oracle_mod, 1e-6), _r(oracle_mod, 1e-6 / 17), 0.0):
        inv, p = cetkmc.implicit_coeffs(L, r)
        winv, wp = implicit_ref.coeffs(L, r)
        assert inv.tobytes() == winv.tobytes() and p.tobytes() == wp.tobytes(), (L, r)
    assert 2.7 < _r(oracle_mod, 1e-6) < 2.73


def test_library_coefficients_refusals():
    import cetkmc
    for L, r, word in ((0, 1.0, "L must be"), (-3, 1.0, "L must be"), (4, np.nan, "not finite"), (4, np.inf, "not finite"),
                       (4, -np.inf, "not finite"), (4, -1e-300, ">= 0")):
        with pytest.raises(ValueError, match="cetkmc_implicit_coeffs") as err:
            cetkmc.implicit_coeffs(L, r)
        assert word in str(err.value)


def test_solve_against_a_dense_matrix(oracle_mod):
    """L = 7, values up to 4100 K: the residual of (I - r D) x = b stays below 1e-10 K along each axis"""
    L = 7
    r = _r(oracle_mod, 1e-6)
    D = -2.0 * np.eye(L) + np.eye(L, k=1) + np.eye(L, k=-1)
    D[0, 0] = D[L - 1, L - 1] = -1.0
    A = np.eye(L) - r * D
    b = np.random.RandomState(0).uniform(0.0, 4100.0, (L, L, L))
    inv, p = implicit_ref.coeffs(L, r)
    worst = 0.0
    for axis in range(3):
        x = implicit_ref.solve(b, axis, r, inv, p)
        res = np.moveaxis(np.tensordot(A, np.moveaxis(x, axis, 0), axes=1), 0, axis) - b
        worst = max(worst, float(np.abs(res).max()))
    print("largest residual", worst)
    assert worst <= 1e-10


def test_one_voxel_is_the_identity_plus_the_source(oracle_mod):
    z = np.zeros((1, 1, 1))
    lat = oracle_mod.Lattice(z.astype(np.int64), z, z, z + 3333.0, impurity_c=0.1)
    implicit_ref.update(lat, 1, 1e-6, 1)
    assert lat.T.tobytes() == (z + 3333.0).tobytes()
    q = np.array([[5e12]])
    implicit_ref.update(lat, 1, 1e-6, 2, q, use_latent=False)
    assert lat.T[0, 0, 0] == 3333.0 + 1e-6 * (q[0, 0] / lat.params.rho_cp + lat.params.latent_coef * 0.0)
    assert 3333.0 < lat.T[0, 0, 0] < ic.CLIP_HI


def test_rough_field_five_updates(oracle_mod):
    """the L = 24 ramp with +- 50 K of noise: no voxel on a clip value (the reference's single step leaves more than 99 %
    there), the range within the input's, the mean unchanged"""
    L = 24
    T0 = sc.noisy_gradient(L, seed=1)
    z = np.zeros((L, L, L))
    lat = oracle_mod.Lattice(z.astype(np.int64), z, z, T0, impurity_c=0.0)
    exp = oracle_mod.Lattice(z.astype(np.int64), z, z, T0, impurity_c=0.0)
    for _ in range(5):
        implicit_ref.update(lat, 1, 1e-6, 1)
        substep_ref.update(exp, 1, 1e-6, 1)
    assert substep_ref.on_clip(lat) == 0.0 and substep_ref.on_clip(exp) > 0.99
    lo, hi = T0.min(), T0.max()
    print("range", lat.T.min() - lo, hi - lat.T.max(), "mean", lat.T.mean() - T0.mean())
    assert lat.T.min() >= lo * (1 - 1e-12) and lat.T.max() <= hi * (1 + 1e-12)
    assert abs(lat.T.mean() - T0.mean()) <= 1e-9


@pytest.mark.parametrize("thermal_mode", [1, 2])
def test_stepper_with_the_explicit_update_is_the_unbroken_oracle_run(oracle_mod, thermal_mode):
    """n = 1 of the chunked Stepper with tests/substep_ref.update substituted: consecutive calls, one stopping with status 2
    ON update step 20 and its continuation, against oracle.Lattice.run_steps on a second lattice"""
    case = dict(rc.STEPPING["L24_laser_latent_rng0_full"], thermal_mode=thermal_mode)
    lat0 = rc.lattice_of(case)
    (s0, n, up, ud, unp, q), = rc.calls_of(dict(case, batches=(45,)))
    a, b = (oracle_mod.Lattice(*lat0, impurity_c=0.1) for _ in range(2))
    st = implicit_ref.Stepper(a, 1, update_fn=substep_ref.update)
    probe = implicit_ref.Stepper(oracle_mod.Lattice(*lat0, impurity_c=0.1), 1, update_fn=substep_ref.update)
    cut = probe.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=thermal_mode, q_planes=q)["np_used"]
    calls = [(0, 30, up, ud, unp[:cut], q), (20, 25, up[20:], ud[20:], unp, None if q is None else q[1:])]
    for c, (g0, m, p, d, u, planes) in enumerate(calls):
        kw = dict(rng_mode=0, thermal_mode=thermal_mode, q_planes=planes)
        ra = st.run_steps(g0, m, 0.1, p, d, u, **kw)
        if c == 1:          # the unbroken oracle has no marker: its continuation starts behind the update it already applied
            kw_b = dict(kw, q_planes=None if planes is None else planes[1:])
            r0 = b.run_steps(g0, 1, 0.1, p[:1], d[:1], u, rng_mode=0, thermal_mode=0)
            r1 = b.run_steps(g0 + 1, m - 1, 0.1, p[1:], d[1:], u[r0["np_used"]:], **kw_b)
            assert (ra["done"], ra["status"]) == (25, 0) and r0["done"] == 1 and r1["done"] == 24
            assert ra["np_used"] == r0["np_used"] + r1["np_used"]
            assert ra["events"].tobytes() == r0["events"].tobytes() + r1["events"].tobytes()
            assert ra["totals"].tobytes() == r0["totals"].tobytes() + r1["totals"].tobytes()
        else:
            rb = b.run_steps(g0, m, 0.1, p, d, u, **kw)
            assert (ra["done"], ra["status"]) == (20, 2)
            for f in ("done", "status", "np_used", "q_used"):
                assert ra[f] == rb[f], f
            for f in ("totals", "events", "n_events"):
                assert ra[f].tobytes() == rb[f].tobytes(), f
        for f in ("state", "theta", "phi", "T", "prev_state"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (c, f)
    assert st.stats["updates"] == 3


@pytest.mark.parametrize("L", ic.SIZES)
def test_direct_inputs_hold_what_they_claim(oracle_mod, L):
    """a latent release and a non-zero source with its peak on the corner; voxels on both clip values after some step (L >= 5:
    smaller lattices have no room for the cold planes beside the beam); NaN, +inf and -inf in front of step 1 of the non-finite
    set, none left with the scrub on; one NaN with the scrub off spreads over the lattice"""
    fields, prev, q = ic.direct_fields(L)
    assert q[0, 0] == q.max() > 0.0
    _, st = ic.direct_reference(L, 2, 2, updates=2)
    assert st["latent"] > 0 and st["source"] == 2 and st["substeps"] == 4
    if L >= 5:
        assert st["on_clip_lo"] > 0 and st["on_clip_hi"] > 0, st
    if L >= 3:
        assert len(ic.nonfinite_sites(L)) >= 4
        T, st = ic.direct_reference(L, 2, 2, nonfinite=True)
        assert st["nan_before"] >= 1 and st["inf_before"] >= 2 and not np.isnan(T).any() and np.isfinite(T).all()
    T, st = ic.direct_reference(L, 2, 1, scrub=False, only_nan=True)
    assert st["nan_before"] == 1 and np.isnan(T).all()        # three full solves: the NaN reaches every voxel


def _assert_run_holds(case, run, tag, steps=True):
    st = run["stepper"].stats
    assert st["updates"] >= 1 and st["substeps"] == st["updates"] * case["n_sub"], tag
    assert st["nan_before"] >= 1 and st["inf_before"] >= 1, (tag, st)            # in front of the first update
    assert st["on_clip_lo"] > 0 and st["on_clip_hi"] > 0, (tag, st)               # after some step
    assert not np.isnan(run["fields"][-1][3]).any(), tag
    if case["thermal_mode"] == 2:
        assert st["source"] == st["updates"], (tag, st)
        if case["use_latent"] and steps:
            assert st["latent"] > 0, (tag, st)
    if steps:
        assert len(run["results"]) == len(run["calls"]) and all(r["status"] == 0 for r in run["results"]), tag
        assert st["updates"] >= 2, tag
        assert all(np.isfinite(r["totals"]).all() for r in run["results"]), tag


@pytest.mark.parametrize("name", list(ic.STEPPING))
def test_stepping_inputs_hold_what_they_claim(oracle_mod, name):
    """every stepping case (L = 136 and 256 included): it begins on an update step; a NaN and a +inf stand in front of that
    update; voxels land on each clip value after some step; at least two updates with the step count of the case; a non-zero
    source and (where the case has latent heat) a release in laser mode; melted voxels where remelting is on; finite totals and
    no stop before the last call"""
    case = ic.STEPPING[name]
    assert case["step0"] % 20 == 0
    run = ic.stepped(name)
    _assert_run_holds(case, run, name)
    if case["remelt"]:
        assert run["stepper"].info["n_melted"] > 0


@pytest.mark.parametrize("name,R", [("ens_L30_n1", 3), ("ens_L33_n3", 70)])
def test_ensemble_inputs_hold_what_they_claim(oracle_mod, name, R):
    """every replica's input of the ensemble test, the empty replica and the one that terminates at once (which makes one
    update and no step) included"""
    case, runs = ic.replica_runs(name, R)
    assert case["step0"] % 20 == 0
    seen = set()
    for r, (run, _) in enumerate(runs):
        if id(run) in seen:
            continue
        seen.add(id(run))
        _assert_run_holds(case, run, (name, r), steps=r != 0)
    cold = runs[0][0]
    assert cold["results"][0]["status"] == 1 and cold["results"][0]["done"] == 0 and cold["stepper"].stats["updates"] == 1
