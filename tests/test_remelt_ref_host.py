"""The remelting comparator (tests/remelt_ref.py) on its own, no GPU: the rule on hand-computed lattices, the chunked
stepping driver against one unbroken oracle call when nothing can melt, and -- for EVERY input of the GPU files
(tests/remelt_cases.py) -- that the input exercises what those tests are about."""
import numpy as np
import pytest

import remelt_cases as rc
from remelt_ref import Stepper, empty_neighbour, remelt

THR = 3695.0


def _lattice(oracle_mod, state, T, theta=None, phi=None):
    state = np.asarray(state, np.int64)
    theta = np.full(state.shape, 0.5) if theta is None else theta
    phi = np.full(state.shape, 1.5) if phi is None else phi
    return oracle_mod.Lattice(state, theta, phi, np.asarray(T, np.float64), np.zeros_like(state), impurity_c=0.1)


def test_rule_on_a_hand_computed_2x2x2_lattice(oracle_mod):
    """eight voxels, one per clause of the rule"""
    below = np.nextafter(THR, -np.inf)
    #         atom on thr  atom below  atom NaN  atom +inf  state 4 hot  empty hot  atom cold  atom hot
    state = [1,            2,          3,        1,         4,           0,         2,         3]
    T = [THR,              below,      np.nan,   np.inf,    4000.0,      4000.0,    3000.0,    3695.5]
    lat = _lattice(oracle_mod, np.reshape(state, (2, 2, 2)), np.reshape(T, (2, 2, 2)))
    lat.defects[0, 0, 0] = 1
    T0, d0 = lat.T.copy(), lat.defects.copy()
    assert remelt(lat, THR) == 4
    assert lat.state.ravel().tolist() == [0, 2, 3, 0, 0, 0, 2, 0]
    assert lat.prev_state.ravel().tolist() == [0, 2, 3, 0, 0, 0, 2, 0]
    assert lat.theta.ravel().tolist() == [0.0, 0.5, 0.5, 0.0, 0.0, 0.5, 0.5, 0.0]      # the hot EMPTY voxel keeps its orientation
    assert lat.phi.ravel().tolist() == [0.0, 1.5, 1.5, 0.0, 0.0, 1.5, 1.5, 0.0]
    assert np.array_equal(lat.T, T0, equal_nan=True) and np.array_equal(lat.defects, d0) and lat.nuc_count == 0
    before = [a.copy() for a in (lat.state, lat.prev_state, lat.theta, lat.phi)]
    assert remelt(lat, THR) == 0                                                       # idempotent on an unchanged field
    assert all(np.array_equal(a, b) for a, b in zip(before, (lat.state, lat.prev_state, lat.theta, lat.phi)))


def test_rule_on_a_hand_computed_3x3x3_lattice(oracle_mod):
    """a hot plane i = 1 in a full lattice: nine voxels melt, prev_state follows although it differed before"""
    state = np.ones((3, 3, 3), np.int64)
    state[1, 1, 1] = 4
    T = np.full((3, 3, 3), 3000.0)
    T[1] = 3800.0
    lat = _lattice(oracle_mod, state, T)
    lat.prev_state[:] = 2                      # a stale prev_state is cleared where the voxel melts, and only there
    assert remelt(lat, THR) == 9
    assert (lat.state[1] == 0).all() and (lat.state[[0, 2]] == 1).all()
    assert (lat.prev_state[1] == 0).all() and (lat.prev_state[[0, 2]] == 2).all()
    assert (lat.theta[1] == 0.0).all() and (lat.theta[[0, 2]] == 0.5).all()
    assert remelt(lat, np.inf) == 0 and remelt(lat, -np.inf) == 18 and (lat.state == 0).all()


def test_empty_neighbour_mask():
    state = np.ones((5, 5, 5), np.int64)
    state[2, 2, 2] = 0
    nb = empty_neighbour(state)
    want = {(2 + a, 2 + b, 2 + c) for a, b, c in ((1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (0, 1, 1), (0, 1, -1), (0, -1, 1),
                                                  (0, -1, -1), (2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2))}
    assert {tuple(v) for v in np.argwhere(nb)} == want


@pytest.mark.parametrize("thermal_mode,rng_mode,step0,batches", [(1, 0, 0, (7, 13, 1, 20, 9)), (2, 1, 19, (23, 5)), (2, 0, 0, (45,)),
                                                                 (1, 2, 15, (30,)), (0, 1, 0, (25,))])
def test_chunked_driver_equals_one_unbroken_oracle_call_when_nothing_melts(oracle_mod, thermal_mode, rng_mode, step0, batches):
    """threshold +inf: the driver's updates, chunks and carried stream positions must reproduce oracle.run_steps (rng_mode
    2: its single-domain super-steps) bit for bit, call after call"""
    case = dict(rc.STEPPING["L24_laser_latent_rng0_full"], thermal_mode=thermal_mode, rng_mode=rng_mode, step0=step0, batches=batches)
    lat0 = rc.lattice_of(case)
    a, b = (oracle_mod.Lattice(*lat0, impurity_c=0.1) for _ in range(2))
    st = Stepper(a, np.inf)
    for (s0, n, up, ud, unp, q) in rc.calls_of(case):
        ra = st.run_steps(s0, n, 0.1, up, ud, unp, rng_mode=rng_mode, seed=9, thermal_mode=thermal_mode, q_planes=q)
        if rng_mode == 2:
            rb = b.run_supersteps(s0, n, b.L, 0.1, 9, thermal_mode=thermal_mode, q_planes=q, want_events=True)
            rb["events"] = rb["events"].reshape(-1)
        else:
            rb = b.run_steps(s0, n, 0.1, up, ud, unp, rng_mode=rng_mode, seed=9, thermal_mode=thermal_mode, q_planes=q)
        assert ra["done"] == rb["done"] == n and ra["status"] == rb["status"] == 0
        for f in ("np_used", "q_used"):
            assert f not in ra or ra[f] == rb[f], f
        for f in ("totals", "events", "n_events", "dt_event"):
            assert f not in ra or np.array_equal(ra[f], rb[f]), f
        for f in ("state", "theta", "phi", "T", "prev_state"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert a.nuc_count == b.nuc_count
    assert st.info["n_melted"] == 0
    assert st.info["passes"] == (sum(1 for g in range(step0, step0 + sum(batches)) if g % 20 == 0) if thermal_mode else 0)


def test_chunked_driver_stream_shortage_on_an_update_step(oracle_mod):
    """status 2 ON an update step and its continuation against the unbroken oracle: the update is applied once"""
    case = rc.STEPPING["L24_laser_latent_rng0_full"]
    lat0 = rc.lattice_of(case)
    a, b = (oracle_mod.Lattice(*lat0, impurity_c=0.1) for _ in range(2))
    (s0, n, up, ud, unp, q), = rc.calls_of(dict(case, batches=(30,)))
    cut = b.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=2, q_planes=q)["np_used"]
    b = oracle_mod.Lattice(*lat0, impurity_c=0.1)
    st = Stepper(a, np.inf)
    for lat_run in (st.run_steps, b.run_steps):
        r = lat_run(0, 30, 0.1, up, ud, unp[:cut], rng_mode=0, thermal_mode=2, q_planes=q)
        assert (r["done"], r["status"], r["q_used"]) == (20, 2, 2)
    assert st.applied_g == 20 and st.info["passes"] == 2
    r1 = st.run_steps(20, 10, 0.1, up[20:], ud[20:], unp, rng_mode=0, thermal_mode=2, q_planes=q[1:])
    assert st.info["passes"] == 2 and (r1["done"], r1["status"], r1["q_used"]) == (10, 0, 1)
    # the oracle's own continuation would update a second time: an unbroken run is the reference for the fields
    c = oracle_mod.Lattice(*lat0, impurity_c=0.1)
    c.run_steps(0, 20, 0.1, up[:20], ud[:20], unp, rng_mode=0, thermal_mode=2, q_planes=q)
    c.thermal_laser(1e-6, q[1], scrub_nan=True)
    rc_ = c.run_steps(20, 10, 0.1, up[20:], ud[20:], unp, rng_mode=0, thermal_mode=0)
    assert np.array_equal(r1["events"], rc_["events"]) and np.array_equal(r1["totals"], rc_["totals"])
    for f in ("state", "theta", "phi", "T", "prev_state"):
        assert np.array_equal(getattr(a, f), getattr(c, f)), f


@pytest.mark.parametrize("name", list(rc.STEPPING) + list(rc.ENSEMBLE))
def test_stepping_inputs_exercise_remelting(oracle_mod, name):
    """on the comparator alone: voxels melt at two or more different updates; a melted voxel is occupied again later (and,
    with latent heat on, in front of an update with prev_state still 0: it changes that update's field); a listed, an interior
    and a state-4 voxel are among the melted ones; no occupied voxel's T lies within 1e-9 relative of the threshold at a
    decision"""
    case = {**rc.STEPPING, **rc.ENSEMBLE}[name]
    run = rc.stepped(name)
    s = run["stepper"].stats
    print(name, s, run["stepper"].info, run["stepper"].min_gap)
    assert all(r["status"] == 0 and r["done"] == c[1] for r, c in zip(run["results"], run["calls"]))
    assert len(set(s["melting"])) >= 2, s
    assert s["refilled"] >= 1, s
    if case["thermal_mode"] == 2 and case["use_latent"]:
        assert s["latent_refills"] >= 1, s
    assert s["listed"] >= 1 and s["interior"] >= 1 and s["state4"] >= 1, s
    assert run["stepper"].min_gap > 1e-9


@pytest.mark.parametrize("L", rc.DIRECT_SIZES)
def test_direct_call_inputs_hold_what_they_claim(oracle_mod, L):
    """the crafted molten sets of the direct-call file: every named voxel is in the lattice it is built into, the equality /
    one-ulp / NaN / +inf voxels and the hot empty voxels behave as the rule says, the plane / whole-lattice / nothing sets
    melt what their names say"""
    for kind in rc.DIRECT_KINDS:
        fields, thr, claim = rc.direct_case(L, kind)
        lat = oracle_mod.Lattice(*fields, impurity_c=0.1)
        s0, th0 = lat.state.copy(), lat.theta.copy()
        k = remelt(lat, thr)
        gone = (s0 != 0) & (lat.state == 0)
        assert int(gone.sum()) == k
        assert all(gone[v] for v in claim["melts"]), kind
        for v in claim["stays"]:
            assert not gone[v] and lat.state[v] == s0[v] and lat.theta[v] == th0[v]
        if kind == "crafted":
            assert k == len(claim["melts"])
        if kind == "plane":
            want = np.zeros_like(gone)
            want[L // 2] = s0[L // 2] != 0
            assert np.array_equal(gone, want)
        if kind == "all":
            assert k == int((s0 != 0).sum()) and (lat.state == 0).all()
        if kind == "nothing":
            assert k == 0
