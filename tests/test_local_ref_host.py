"""The comparator of Mode B's local event loop (tests/local_ref.py) on its own, no device: with one event per box and an
infinite horizon it is the oracle's orc_run_supersteps without null events; a one-atom lattice is followed by hand, key by
key; and the inputs of the GPU comparison exercise what that comparison is meant to cover."""
import math

import numpy as np
import pytest

import local_ref as LR
from helpers import random_lattice


@pytest.mark.parametrize("L,fill,df,thermal_mode", [(16, 0.2, 0.05, 1), (24, 0.02, 0.02, 1), (32, 0.3, 0.1, 0)])
def test_one_event_and_no_horizon_is_mode_b_without_null_events(oracle_mod, L, fill, df, thermal_mode):
    fields = random_lattice(L, 100 + L, fill=fill)
    a = oracle_mod.Lattice(*fields, impurity_c=0.2)
    b = oracle_mod.Lattice(*fields, impurity_c=0.2)
    step = 5
    for n in (11, 13):
        ra = LR.run(oracle_mod, a, step, n, df, 4242, 1, math.inf, thermal_mode=thermal_mode)
        rb = b.run_supersteps(step, n, 8, df, 4242, thermal_mode=thermal_mode, null_events=False)
        assert ra["done"] == rb["done"] == n and ra["status"] == rb["status"] == 0
        assert ra["events"].shape == (n, (L // 8) ** 3, 1)
        for f in ("type", "pos", "target", "atom", "rate", "dep_rank"):
            assert np.array_equal(ra["events"][f][:, :, 0], rb["events"][f]), f
        assert np.array_equal(ra["totals"], rb["totals"]) and np.array_equal(ra["dt_event"], rb["dt_event"])
        assert np.array_equal(ra["n_exec"], rb["n_exec"])
        assert np.array_equal(ra["n_capped"], rb["n_exec"])            # a box that executes max_events events is capped
        assert np.all(np.isinf(ra["horizon"]))
        for f in ("state", "theta", "phi", "T"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert a.nuc_count == b.nuc_count
        step += n
    assert ra["n_exec"].max() > 1


def test_one_atom_by_hand(oracle_mod):
    """8^3, one tungsten atom at (1, 2, 1), 3000 K everywhere, I0 lowered so that the atom's events carry the window: one
    box whose octant-0 window [0, 4)^3 holds the atom.  Super-step 0 is replayed here with the keys spelled out."""
    L, seed, K, hor = 8, 31, 3, 2.5
    state = np.zeros((L, L, L), np.int64)
    state[1, 2, 1] = 1
    theta = np.where(state == 1, 0.7, 0.0)
    phi = np.where(state == 1, 1.9, 0.0)
    T = np.full((L, L, L), 3000.0)

    def lattice():
        lat = oracle_mod.Lattice(state, theta, phi, T, None, impurity_c=0.2)
        lat.params.I0 = 1e9
        return lat
    lat = lattice()
    r = LR.run(oracle_mod, lat, 0, 1, 0.0, seed, K, hor, thermal_mode=0)
    ev = r["events"][0, 0]
    # by hand, on a second copy
    ref = lattice()
    u = oracle_mod.counter_uniform
    pick, R = ref.window_pick(0, 0, 0, 4, u(seed, 0, (1 << 40) | 0), with_total=True)
    assert pick is not None and r["horizon"][0] == hor / R
    tau, t, m = hor / R, 0.0, 0
    while pick is not None and m < K:
        w = -math.log(u(seed, 0, (7 << 40) | (m << 24) | 0)) / R
        if t + w > tau:
            break
        t += w
        assert (ev[m]["type"], tuple(ev[m]["pos"]), tuple(ev[m]["target"])) == (pick.type, tuple(pick.pos), tuple(pick.target))
        assert ev[m]["rate"] == pick.rate
        th = ph = 0.0
        if pick.type in (0, 2):
            th = math.pi * u(seed, 0, (2 << 40) | (m << 24) | 0)
            ph = 2 * math.pi * u(seed, 0, (3 << 40) | (m << 24) | 0)
            assert (ev[m]["theta"], ev[m]["phi"]) == (th, ph)
        ref.apply(pick, th, ph, False)
        m += 1
        if m < K:
            pick, R = ref.window_pick(0, 0, 0, 4, u(seed, 0, (1 << 40) | (m << 24) | 0), with_total=True)
    assert m == r["n_exec"][0] >= 2 and np.all(ev["type"][m:] == -1) and np.all(ev["target"][m:] == -1)
    assert r["n_capped"][0] == int(m == K)
    assert set(ev["type"][:m]) <= {1, 2, 3} and (ev["type"][:m] != 2).any()     # the atom's own events take part
    assert np.array_equal(ref.state, lat.state) and np.array_equal(ref.theta, lat.theta)
    assert LR.keys(2, 5, 3, 4, 8) == dict(wait=(7 << 40) | (2 << 24) | 5, pick=(1 << 40) | (2 << 24) | 5, theta=(2 << 40) | (2 << 24) | 5,
                                          phi=(3 << 40) | (2 << 24) | 5, defect=(4 << 40) | (2 << 24) | 5, species=(2 << 44) | 28)
    assert LR.keys(0, 5, 3, 4, 8)["species"] == 28 and LR.keys(0, 5, 3, 4, 8)["pick"] == oracle_mod.KEY_PICK | 5


def _coverage(oracle_mod, name):
    kinds, stops, outside, margin, most = [0, 0, 0, 0], dict.fromkeys(LR.STOPS, 0), 0, math.inf, 0
    for r, *_ in LR.reference_run(oracle_mod, name):
        s = r["stats"]
        kinds = [a + b for a, b in zip(kinds, s["kinds_later"])]
        for k in LR.STOPS:
            stops[k] += s["stops"][k]
        outside += s["targets_outside"]
        margin = min(margin, s["min_margin"])
        most = max(most, s["max_per_box"])
    return kinds, stops, outside, margin, most


@pytest.mark.parametrize("name", list(LR.INPUTS))
def test_every_gpu_input_covers_the_loop(oracle_mod, name):
    """Every input of the GPU files: boxes with >= 3 events, both stops, nucleation / attachment / diffusion at m >= 1, a
    diffusion target outside its window, and no horizon decision closer to the horizon than 1e-6 (device and comparator
    rates may differ by 1e-11).  Only the horizon stop is exempt where the horizon is infinite: it cannot occur there."""
    kinds, stops, outside, margin, most = _coverage(oracle_mod, name)
    assert most >= 3, most                                             # boxes with >= 3 events
    assert stops["capped"] > 0 and (stops["horizon"] > 0) == (name not in LR.NO_HORIZON), stops
    assert kinds[2] > 0 and kinds[3] > 0 and kinds[1] > 0, kinds      # nucleation, attachment, diffusion at m >= 1
    assert outside >= 1
    assert margin >= 1e-6, margin


def test_a_deposition_follows_an_earlier_event_of_its_box(oracle_mod):
    assert max(_coverage(oracle_mod, name)[0][0] for name in LR.TABLE) > 0


def test_runs_without_a_horizon(oracle_mod):
    """Cap 64 = the window: boxes run to the cap or empty their windows until the lattice is full -- the first batch ends
    with status 1 and the second is empty (the GPU comparison checks that stop, nothing more, in its second batch).  Cap 8:
    the same path through both batches in full, the second starting mid-cadence and mid-octant."""
    _, stops, _, _, most = _coverage(oracle_mod, "L16_to_the_cap")
    runs = LR.reference_run(oracle_mod, "L16_to_the_cap")
    assert stops["emptied"] > 0 and most == 64
    assert runs[0][0]["status"] == 1 and runs[0][0]["done"] < LR.BATCHES[0] and runs[1][0]["done"] == 0
    _, stops, _, _, most = _coverage(oracle_mod, "L16_no_horizon")
    runs = LR.reference_run(oracle_mod, "L16_no_horizon")
    assert most == 8 and [r[0]["done"] for r in runs] == list(LR.BATCHES) and all(r[0]["status"] == 0 for r in runs)
    assert runs[1][0]["n_capped"].sum() > 0
