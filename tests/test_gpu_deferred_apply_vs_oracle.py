"""The default full-sweep batched path at 128 < L <= 256 against the oracle.

There a deferred step launches its selection alone (k_select_pend), the next rate sweep applies the event in an extra
workgroup (k_sweep_stream_apply), re-evaluates the stale rows into a RowPatch and k_plane_reduce substitutes them.  The
on/off tests of test_gpu_apply_in_sweep.py compare that path with the immediate one, which shares the selection, the apply
body, the rate table and the row reduction with it; here the engine runs with its defaults (no set_option) and is
compared with the oracle after EVERY call: stop state, stream positions, event log, totals, all five fields and the row
sums of the lattice the call left.  cetkmc_counters.deferred_steps proves the deferred path was the one that ran.

With the default I0 = 5e13 nearly every chosen event is a nucleation or a deposition; FOUR_KIND_PARAMS (I0 = 1e11) lets
diffusion (two changed sites, patches of more than 11 rows) and attachment fire too.  What the deferred steps exercised
is computed from the ORACLE's log and asserted, so the inputs cannot drift into a run that no longer covers them."""
import os

import numpy as np
import pytest

from helpers import (APPLY_IN_SWEEP_BATCHES, FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, count_deferred,
                     deferred_coverage, face_lattice, oracle_lattice, step_uniforms)
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05


def _run_both(oracle_mod, L, lat, calls, tweak, rng_mode=1, engine_kw=None, run_kw=None):
    """The same calls on a default engine and on the oracle, compared after every call.  Returns (oracle logs, engine
    counters)."""
    import cetkmc
    from cetkmc import synthetic
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in (tweak or {}).items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params, **(engine_kw or {}))
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, tweak)
    logs = []
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(calls):
            q = synthetic.laser_planes(L, step0, n)
            rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, rng_mode=rng_mode, seed=5, thermal_mode=2, q_planes=q,
                             **(run_kw or {}))
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, rng_mode=rng_mode, seed=5, thermal_mode=2, q_planes=q)
            logs.append(ro)
            assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"L={L} call {c} (steps {step0}..{step0 + n - 1})")
    finally:
        oracle_mod.set_threads(1)
    cnt = e.counters()
    e.close()
    return logs, cnt


@pytest.mark.parametrize("L", [129, 200, 256])
def test_four_kinds_vs_oracle(oracle_mod, L):
    """The first size on the path, a ragged row length and the benchmark size; batches starting and ending at many offsets
    modulo 20 plus one of 37 steps; defect injection; all four event kinds on deferred steps."""
    lat = face_lattice(L, 17 + L, 6000)
    calls = batch_calls(APPLY_IN_SWEEP_BATCHES + (37,))
    logs, cnt = _run_both(oracle_mod, L, lat, calls, FOUR_KIND_PARAMS)
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    cov = deferred_coverage(L, calls, logs, DEFECT_FRACTION)
    print(f"L={L} deferred-step coverage (oracle log): {cov}")
    assert min(cov["kinds"]) >= 3, cov                       # deposition, diffusion, nucleation, attachment
    assert cov["diff_rows"] >= 2, cov                        # second site adds rows to the patch
    assert L < 200 or cov["diff_planes"] >= 1, cov
    assert cov["face_i"] >= 1 and cov["face_j"] >= 1, cov    # clipped patches
    assert cov["defects"] >= 1, cov
    assert cnt["deferred_steps"] == count_deferred(calls) == 113
    assert cnt["incremental_steps"] == 0


def test_default_parameters_256_vs_oracle(oracle_mod):
    """What a user gets at the benchmark size: default parameters (nucleation and deposition dominate), temperature
    updates inside and at the edge of a batch, 1-step batches."""
    L = 256
    lat = face_lattice(L, 17 + L, 6000)
    calls = batch_calls(APPLY_IN_SWEEP_BATCHES[:5])
    logs, cnt = _run_both(oracle_mod, L, lat, calls, None)
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    cov = deferred_coverage(L, calls, logs, DEFECT_FRACTION)
    print(f"L={L} default parameters, deferred-step coverage (oracle log): {cov}")
    assert cov["kinds"][0] >= 3 and cov["kinds"][2] >= 3, cov
    assert cnt["deferred_steps"] == count_deferred(calls)


def test_reference_stream_shortage_and_continuation_vs_oracle(oracle_mod):
    """rng_mode 0: one species uniform per deposition candidate, the chosen deposition's dep_rank picks its own.  The batch
    runs out of stream (status 2) behind deferred steps; the continuation resumes at the step it stopped at."""
    L, n, n2 = 160, 30, 30
    lat = face_lattice(L, 5, 3000)
    u_pick, u_def, u_np = step_uniforms(7, n + n2, 9 * (L * L + 2))
    u_np2 = np.random.RandomState(8).random_sample(40 * (L * L + 2))
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    from cetkmc import synthetic
    done = o.run_steps(0, n, DEFECT_FRACTION, u_pick[:n], u_def[:n], u_np, rng_mode=0, seed=5, thermal_mode=2,
                       q_planes=synthetic.laser_planes(L, 0, n))["done"]
    assert 0 < done < n
    calls = [(0, n, u_pick[:n], u_def[:n], u_np), (done, n2, u_pick[done:done + n2], u_def[done:done + n2], u_np2)]
    logs, cnt = _run_both(oracle_mod, L, lat, calls, FOUR_KIND_PARAMS, rng_mode=0)
    assert (logs[0]["done"], logs[0]["status"]) == (done, 2)
    assert (logs[1]["done"], logs[1]["status"]) == (n2, 0)
    cov = deferred_coverage(L, calls, logs, DEFECT_FRACTION)
    print(f"L={L} reference stream, deferred-step coverage (oracle log): {cov}")
    assert cov["kinds"][0] >= 3, cov                         # depositions whose species comes from u_np[pos + dep_rank]
    assert cnt["deferred_steps"] == count_deferred(calls)    # launches issued: the stopped batch counts whole


@pytest.mark.parametrize("L,engine_kw,run_kw", [
    (128, {}, {}),                                  # L <= 128 takes the one-launch small-lattice sweep
    (264, {}, {}),                                  # rows of more than 256 voxels
    (200, {"n_slabs": 2}, {}),
    (200, {}, {"incremental": True}),
], ids=["L128", "L264", "two_slabs", "incremental"])
def test_neighbours_do_not_defer_and_match_oracle(oracle_mod, L, engine_kw, run_kw):
    """The sizes and modes beside the deferring path: same comparison, and the counter stays 0."""
    lat = face_lattice(L, 17 + L, 6000)
    calls = batch_calls((7, 5))
    logs, cnt = _run_both(oracle_mod, L, lat, calls, FOUR_KIND_PARAMS, engine_kw=engine_kw, run_kw=run_kw)
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    assert cnt["deferred_steps"] == 0
    assert cnt["steps"] == 12
