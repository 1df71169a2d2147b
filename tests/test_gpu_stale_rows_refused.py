"""A deferred step that ends the batch: the stream of orientation draws (np_cap) runs out at a step whose selection was
launched alone.

The tiles of the next sweep launch decide from the pending record which rows they leave to the apply block, so the record
and what the apply block does with it must agree also when nothing is applied.  When the stream runs out the selection
sets status 2 and the record names no event (type -1): no row is stale, and the launches behind it return at their status
check.  Status, logs, the row sums of a sweep of the lattice the call left and the lattice itself must equal the
immediate path's and the oracle's, and a continuation call from the stopped step (first launch: a plain sweep over rows
the stopped call last wrote through the deferred path) must too."""
import numpy as np
import pytest

from helpers import assert_call_matches_oracle, is_deferred, oracle_lattice, step_uniforms
from test_gpu_parity import RATE_RTOL
from test_gpu_stale_rows_seams import DEFECT_FRACTION, IMPURITY_C, TWEAK, _engine, _observed, window_lattice

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n_draws", [4, 10])
def test_stream_runs_out_on_a_deferred_step(oracle_mod, n_draws):
    L, seed, n, n2 = 129, 2, 25, 6
    lat = window_lattice(L, seed)
    u_pick, u_def, _ = step_uniforms(300 + seed * 10, n + n2, 2)
    u_np = np.random.RandomState(77).random_sample(n_draws)          # two draws per deposition / nucleation
    u_np2 = np.random.RandomState(78).random_sample(2 * n2 + 2)
    kw = dict(rng_mode=1, seed=5, thermal_mode=0)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, TWEAK)
    on, off = _engine(L, lat, True), _engine(L, lat, False)
    ro = o.run_steps(0, n, DEFECT_FRACTION, u_pick[:n], u_def[:n], u_np, **kw)
    done = ro["done"]
    # the reference run stops for lack of stream, behind at least one deferred step and at a deferred step
    assert ro["status"] == 2 and 1 <= done < n - 1 and is_deferred(0, n, done, 0), (ro["status"], done)
    assert sum(int(t) in (0, 2) for t in ro["events"]["type"][:done]) == n_draws // 2
    ra = on.run_steps(0, n, DEFECT_FRACTION, u_pick[:n], u_def[:n], u_np, **kw)
    rb = off.run_steps(0, n, DEFECT_FRACTION, u_pick[:n], u_def[:n], u_np, **kw)
    assert (ra["done"], ra["status"]) == (rb["done"], rb["status"]) == (done, 2)
    a, b = _observed(on, ra), _observed(off, rb)
    for q, (x, y) in enumerate(zip(a, b)):
        assert x == y, f"stopped call: item {q} of the observed state differs between the deferred and the immediate path"
    assert_call_matches_oracle(on, o, ra, ro, RATE_RTOL, tag="stopped call, apply_in_sweep on")
    # continuation from the stopped step with a fresh stream
    args = (done, n2, DEFECT_FRACTION, u_pick[done:done + n2], u_def[done:done + n2], u_np2)
    ro2 = o.run_steps(*args, **kw)
    ra2, rb2 = on.run_steps(*args, **kw), off.run_steps(*args, **kw)
    assert (ra2["done"], ra2["status"]) == (rb2["done"], rb2["status"]) == (n2, 0)
    a, b = _observed(on, ra2), _observed(off, rb2)
    for q, (x, y) in enumerate(zip(a, b)):
        assert x == y, f"continuation: item {q} of the observed state differs between the deferred and the immediate path"
    assert_call_matches_oracle(on, o, ra2, ro2, RATE_RTOL, tag="continuation, apply_in_sweep on")
    assert on.counters()["deferred_steps"] == (n - 1) + (n2 - 1) and off.counters()["deferred_steps"] == 0
    on.close()
    off.close()
