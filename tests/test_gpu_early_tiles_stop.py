"""Option early_tiles: the uniform stream runs out on a deferred step whose selection launch carries early tiles.

rng_mode 0 (one species uniform per deposition candidate): the selection of a deferred step notices the shortage and stops the
batch (status 2) in the very launch whose other blocks are storing the next step's rows into the other row-sum pair.  Those
tiles read no step status; the launches queued behind the stop pass through, the host has flipped the pair once per queued
deferred step, and the pairs hold 0xFF bytes from poison_alt_rows wherever nothing was stored.  The stop, the status, the
downloaded lattice, the row sums read back afterwards (cetkmc_row_sums behind a sweep of the lattice as it stands) and the
continuation in a second call must equal early_tiles = 0 bit for bit, and the oracle (the scenario of
test_gpu_deferred_apply_vs_oracle.test_reference_stream_shortage_and_continuation_vs_oracle)."""
import os

import numpy as np
import pytest

from helpers import (FOUR_KIND_PARAMS, assert_call_matches_oracle, count_deferred, face_lattice, is_deferred, oracle_lattice,
                     step_uniforms)
from test_gpu_early_tiles import _engine, frozen, tile_count
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05


def _observed(e, r):
    d = e.download(defects=True)
    info = e.rate_sweep()
    rs, rc = e.row_sums()
    return (r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["totals"][:r["done"]].tobytes(),
            r["events"][:r["done"]].tobytes(), r["n_events"][:r["done"]].tobytes(), info, rs.tobytes(), rc.tobytes()) + \
        tuple(d[k].tobytes() for k in sorted(d))


def test_stream_runs_out_on_a_step_with_early_tiles(oracle_mod):
    from cetkmc import synthetic
    L, n, n2 = 160, 30, 30
    lat = face_lattice(L, 5, 3000)
    u_pick, u_def, u_np = step_uniforms(7, n + n2, 9 * (L * L + 2))
    u_np2 = np.random.RandomState(8).random_sample(40 * (L * L + 2))
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    variants = (0, 8 * (tile_count(L) // 16), tile_count(L))
    engines = {v: _engine(L, lat, v) for v in variants}
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        kw = dict(rng_mode=0, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, 0, n))
        ro = o.run_steps(0, n, DEFECT_FRACTION, u_pick[:n], u_def[:n], u_np, **kw)
        done = ro["done"]
        assert ro["status"] == 2 and 0 < done < n and is_deferred(0, n, done), (done, ro["status"])     # the step that stops is a deferred one
        calls = [(0, n, u_pick[:n], u_def[:n], u_np), (done, n2, u_pick[done:done + n2], u_def[done:done + n2], u_np2)]
        for c, (step0, m, up, ud, un) in enumerate(calls):
            kw = dict(rng_mode=0, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, step0, m))
            if c:
                ro = o.run_steps(step0, m, DEFECT_FRACTION, up, ud, un, **kw)
                assert (ro["done"], ro["status"]) == (n2, 0)
            left = frozen(o)
            seen = {}
            for v, e in engines.items():
                rg = e.run_steps(step0, m, DEFECT_FRACTION, up, ud, un, **kw)
                seen[v] = _observed(e, rg)
                assert_call_matches_oracle(e, left, rg, ro, RATE_RTOL, tag=f"call {c}, early_tiles {v}")
            for v in variants[1:]:
                for q, (x, y) in enumerate(zip(seen[0], seen[v])):
                    assert x == y, f"call {c}: item {q} of the observed state differs between early_tiles 0 and {v}"
    finally:
        oracle_mod.set_threads(1)
    n_def = count_deferred(calls)
    for v, e in engines.items():
        cnt = e.counters()
        assert cnt["deferred_steps"] == n_def and cnt["early_tiles"] == n_def * v, (v, cnt)      # launches issued: the stopped batch counts whole
        e.close()
