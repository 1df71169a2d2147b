"""Mode B's local event loop on the device (cetkmc_run_supersteps_local, csrc/local.hpp) against its comparator
(tests/local_ref.py): the per-box event sequences, executed and capped counts, horizons, totals and every lattice field
after each of two batches; then the state the loop leaves behind for the other stepping modes.  The comparisons follow
tests/test_gpu_mode_b.py.  What the inputs exercise is asserted in tests/test_local_ref_host.py."""
import numpy as np
import pytest

import local_ref as LR
from helpers import assert_call_matches_oracle, assert_supersteps_match_oracle, relerr

pytestmark = pytest.mark.gpu
RATE_RTOL = 1e-11


def _engine(name):
    import cetkmc
    L = LR.INPUTS[name][0]
    fields, _, tweak = LR.make_input_fields(name)
    params = cetkmc.default_params(LR.IMPURITY_C)
    for k, v in tweak.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=LR.IMPURITY_C, params=params)
    e.upload(*fields)
    return e


@pytest.mark.parametrize("name", list(LR.INPUTS))
def test_local_loop_vs_comparator(oracle_mod, name):
    # (L16_to_the_cap fills the lattice within its first batch: that batch ends with status 1 and a terminating total, and
    # the second batch compares that nothing runs any more; L16_no_horizon carries the cap path through both batches)
    L, _, _, hor, K, _, tm, df = LR.INPUTS[name]
    e = _engine(name)
    step = LR.STEP0
    for n, (ro, state, theta, phi, T, nuc) in zip(LR.BATCHES, LR.reference_run(oracle_mod, name)):
        rg = e.run_supersteps_local(step, n, df, LR.SEED, K, hor, thermal_mode=tm, want_events=True)
        print(name, "batch", n, "done", rg["done"], ro["done"], "executed", int(rg["n_exec"].sum()), int(ro["n_exec"].sum()),
              "capped", int(rg["n_capped"].sum()), int(ro["n_capped"].sum()))
        assert rg["done"] == ro["done"] and rg["status"] == ro["status"]
        done = ro["done"]
        ge, oe = rg["events"], ro["events"]
        assert ge.shape == oe.shape == (done, (L // 8) ** 3, K)
        for f in ("type", "pos", "target", "atom"):
            if not np.array_equal(ge[f], oe[f]):
                bad = np.argwhere((ge[f] != oe[f]).reshape(done, ge.shape[1], K, -1).any(axis=3))[0]
                raise AssertionError(f"{name}: event field {f} differs first at super-step {bad[0]} of the batch, box {bad[1]}, "
                                     f"event {bad[2]}: engine {ge[tuple(bad)]} comparator {oe[tuple(bad)]}")
        live = oe["type"] >= 0
        if live.any():
            assert relerr(ge["rate"][live], oe["rate"][live]).max() <= RATE_RTOL
            assert np.array_equal(ge["theta"][live], oe["theta"][live]) and np.array_equal(ge["phi"][live], oe["phi"][live])
        assert np.array_equal(rg["n_exec"], ro["n_exec"]) and np.array_equal(rg["n_capped"], ro["n_capped"])
        assert len(rg["totals"]) == len(ro["totals"])
        if len(ro["totals"]):
            assert relerr(rg["totals"], ro["totals"]).max() <= RATE_RTOL
        if done:
            fin = np.isfinite(ro["horizon"])
            assert np.array_equal(np.isfinite(rg["horizon"]), fin) and np.array_equal(rg["horizon"][~fin], ro["horizon"][~fin])
            if fin.any():
                assert relerr(rg["horizon"][fin], ro["horizon"][fin]).max() <= RATE_RTOL
            assert relerr(rg["dt_event"], ro["dt_event"]).max() <= RATE_RTOL
        d = e.download()
        assert np.array_equal(d["state"], state)
        assert np.array_equal(d["theta"], theta) and np.array_equal(d["phi"], phi)
        assert np.array_equal(d["T"], T)
        assert rg["nucleation_count"] == nuc
        step += n
    # the engine is in a consistent state for Mode A afterwards (interface list, class array, rate table)
    e.set_option("sweep_variant", 0)
    a = (e.rate_sweep(),) + tuple(x.tobytes() for x in e.row_sums())
    e.set_option("sweep_variant", 1)
    b = (e.rate_sweep(),) + tuple(x.tobytes() for x in e.row_sums())
    assert a == b
    e.close()


def test_derived_state_serves_the_other_modes(oracle_mod):
    """After the loop: 12 null-event super-steps (table-driven picks over the rate table and class bytes the upkeep left)
    and 25 Mode A steps (interface list, neighbourhood words), each against the oracle continuing from the comparator's
    lattice."""
    name = "L16_four_kinds"
    L, _, _, hor, K, _, tm, df = LR.INPUTS[name]
    e = _engine(name)
    _, lat, _ = LR.make_input(oracle_mod, name)
    step = LR.STEP0
    for n in LR.BATCHES:
        e.run_supersteps_local(step, n, df, LR.SEED, K, hor, thermal_mode=tm)
        LR.run(oracle_mod, lat, step, n, df, LR.SEED, K, hor, thermal_mode=tm)
        step += n
    rg = e.run_supersteps(step, 12, 8, df, seed=77, thermal_mode=1, want_events=True, null_events=True)
    ro = lat.run_supersteps(step, 12, 8, df, 77, thermal_mode=1, null_events=True)
    assert_supersteps_match_oracle(e, lat, rg, ro, RATE_RTOL, "null-event super-steps after the local loop")
    step += 12
    rs = np.random.RandomState(9)
    n = 25
    u_pick, u_def, u_np = rs.random_sample(n), rs.random_sample(n), rs.random_sample(2 * n + 2)
    ra = e.run_steps(step, n, df, u_pick, u_def, u_np, rng_mode=1, seed=5, thermal_mode=1)
    rb = lat.run_steps(step, n, df, u_pick, u_def, u_np, rng_mode=1, seed=5, thermal_mode=1)
    assert_call_matches_oracle(e, lat, ra, rb, RATE_RTOL, "Mode A steps after the local loop")
    e.close()
