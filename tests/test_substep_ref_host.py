"""The comparator of the sub-stepping tests (tests/substep_ref.py) and their inputs (tests/substep_cases.py), without a device:
the chunked stepper at n = 1 is the oracle's unbroken run, stable_substeps is 17 for the defaults, the explicit update is
unstable at n = 1 and stable at n = 17 on the rough field of DESIGN.md section 25, and every input of the GPU files holds what
it is meant to exercise."""
import numpy as np
import pytest

import remelt_cases as rc
import substep_cases as sc
import substep_ref


def _same_results(a, b):
    for f in ("done", "status", "np_used", "q_used"):
        assert a[f] == b[f], (f, a[f], b[f])
    for f in ("totals", "events", "n_events"):
        assert a[f].tobytes() == b[f].tobytes(), f


@pytest.mark.parametrize("thermal_mode", [1, 2])
def test_stepper_at_n1_is_the_unbroken_oracle_run(oracle_mod, thermal_mode):
    """consecutive calls, one of them stopping with status 2 ON update step 20 (the stream runs out behind that step's
    update) and its continuation, against oracle.Lattice.run_steps on a second lattice"""
    case = dict(rc.STEPPING["L24_laser_latent_rng0_full"], thermal_mode=thermal_mode)
    lat0 = rc.lattice_of(case)
    (s0, n, up, ud, unp, q), = rc.calls_of(dict(case, batches=(45,)))
    a, b = (oracle_mod.Lattice(*lat0, impurity_c=0.1) for _ in range(2))
    st = substep_ref.Stepper(a, 1)
    probe = substep_ref.Stepper(oracle_mod.Lattice(*lat0, impurity_c=0.1), 1)
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
            _same_results(ra, rb)
        for f in ("state", "theta", "phi", "T", "prev_state"):
            assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (c, f)
    assert st.stats["updates"] == 3 and st.stats["substeps"] == 3


def test_stable_substeps():
    from thermal_solver import ALPHA, stable_substeps
    from constants import VOXEL_SIZE
    assert 6.0 * ALPHA * 1e-6 / VOXEL_SIZE ** 2 > 16.0
    assert stable_substeps(1e-6) == 17 == int(np.ceil(6 * 2.716))
    assert ALPHA * (1e-6 / 17) / VOXEL_SIZE ** 2 <= 1 / 6 < ALPHA * (1e-6 / 16) / VOXEL_SIZE ** 2
    # an exact boundary: alpha = dx = 1, dt = 1/2 gives 1/6 at n = 3 exactly
    assert stable_substeps(0.5, alpha=1.0, dx=1.0) == 3
    assert stable_substeps(np.nextafter(0.5, 0.0), alpha=1.0, dx=1.0) == 3
    assert stable_substeps(np.nextafter(0.5, 1.0), alpha=1.0, dx=1.0) == 4
    assert stable_substeps(1.0 / 6.0, alpha=1.0, dx=1.0) == 1 and stable_substeps(1e-9) == 1
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            stable_substeps(bad)


def test_explicit_update_is_unstable_at_n1_and_stable_at_n17(oracle_mod):
    """an L = 24 linear gradient with +- 50 K of noise through five updates: at n = 1 more than 99 % of the voxels sit on a
    clip value, at n = 17 none does and the +- 50 K of noise have decayed below a kelvin within every plane"""
    L = 24
    T0 = sc.noisy_gradient(L, seed=1)
    z = np.zeros((L, L, L))
    share = {}
    for n in (1, 17):
        lat = oracle_mod.Lattice(z.astype(np.int64), z, z, T0, impurity_c=0.0)
        for _ in range(5):
            substep_ref.update(lat, n, 1e-6, 1)
        share[n] = substep_ref.on_clip(lat)
        if n == 17:
            assert substep_ref.max_inplane_difference(lat.T) < 1.0
    assert share[1] > 0.99 and share[17] == 0.0, share


@pytest.mark.parametrize("L", sc.SMALL_SIZES + sc.LARGE_SIZES[-1:])
def test_direct_inputs_hold_what_they_claim(oracle_mod, L):
    """the direct-call inputs: a latent release and a non-zero source in laser mode, voxels on both clip values after some
    sub-step (L >= 5: a one-voxel lattice cannot span the range), NaN and +inf in front of sub-step 1 of the non-finite set,
    NaN left behind only with the scrub off"""
    fields, prev, q = sc.direct_fields(L)
    assert q[0, 0] == q.max() > 0.0                                      # the peak on the corner
    _, st = sc.direct_reference(L, 5, 2, updates=2, threads=16 if L > 100 else 1)
    assert st["latent"] > 0 and st["source"] == 2 and st["substeps"] == 10
    if L >= 5:
        assert st["on_clip_lo"] > 0 and st["on_clip_hi"] > 0, st
    if L in (5, sc.TJ + 1):
        sites = sc.nonfinite_sites(L)
        assert len(sites) >= 4
        for scrub in (False, True):
            T, st = sc.direct_reference(L, 6, 1, scrub=scrub, nonfinite=True)
            assert st["nan_before"] >= 2 and st["inf_before"] >= 2
            assert bool(np.isnan(T).any()) == (not scrub)
            if not scrub and L > 20:     # the NaN has spread n = 6 cells from its site, and no further
                i, j, k = next(v for q_, v in enumerate(sites) if q_ % 2 == 0 and v[2] + 7 < L)
                assert np.isnan(T[i, j, k + 6]) and not np.isnan(T[i, j, k + 7])


@pytest.mark.parametrize("name", [n for n in {**sc.STEPPING, **sc.ENSEMBLE} if not n.startswith(("L136", "L256"))])
def test_stepping_inputs_hold_what_they_claim(oracle_mod, name):
    """the stepping cases: at least two updates, the sub-step count of the case, a source and (where the case has latent heat)
    a release in laser mode, melted voxels where remelting is on; no stop before the last call"""
    case = {**sc.STEPPING, **sc.ENSEMBLE}[name]
    run = sc.stepped(name)
    st = run["stepper"]
    assert len(run["results"]) == len(run["calls"]) and all(r["status"] == 0 for r in run["results"])
    assert st.stats["updates"] >= 2 and st.stats["substeps"] == st.stats["updates"] * case["n_sub"]
    if case["thermal_mode"] == 2:
        assert st.stats["source"] == st.stats["updates"]
        if case["use_latent"]:
            assert st.stats["latent"] > 0
    if case["remelt"]:
        assert st.melted > 0
