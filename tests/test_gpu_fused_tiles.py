"""Option fused_tiles: the census-free tiles of the streaming sweep launches at 128 < L <= 256 against the ring tiles, bit for
bit, and each against the oracle.

fused_tiles 1 (default): the launch that applies a pending event (k_sweep_stream_apply) reduces its rows with the census-free row_reduce() --
own class byte + rate table, no neighbour census, no LDS ring -- in tiles of consecutive items; fused_tiles 2 gives the plain
launch (k_sweep_stream: temperature-update steps, immediate steps) the same tiles; fused_tiles 0 is the ring tiles in both.
thermal_mode 2 over two temperature updates, in two calls: fused steps, the cold plain sweep behind an update, the immediate
step before an update and a call's last (immediate) step all occur.

L = 129 is the first L on the deferred path, odd (the last row pair is half empty, planes do not divide into whole tiles:
65 pairs per plane, 1049 tiles of 8 items); L = 160 has 1600 tiles, a multiple of 8, so the tiles are renumbered into contiguous
ranges per XCD; L = 256 is the benchmark's size, once.

What the deferred steps exercised is counted from the ORACLE's log.  The inputs below were checked with the oracle alone on
the CPU: all four event kinds occur on deferred steps at every size (the counts are in the test's docstring)."""
import os

import numpy as np
import pytest

from helpers import (FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, count_deferred, deferred_coverage, face_lattice,
                     oracle_lattice)
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
BATCHES = (24, 21)                 # steps 0..44: temperature updates at steps 20 and 40, one inside each call
N_ATOMS = {129: 6000, 160: 6000, 256: 24000}      # impurity atoms strewn into the melt: about the same density at 160 and 256


def inputs(L):
    return face_lattice(L, 17 + L, N_ATOMS[L]), batch_calls(BATCHES)


def _engine(L, lat, fused):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.set_option("fused_tiles", fused)
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


def _observed(e, r):
    """the event log, the totals, the candidate counts, the stream positions and the final fields of a call"""
    d = e.download(defects=True)
    return (r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["full_sweeps"], r["totals"].tobytes(),
            r["events"].tobytes(), r["n_events"].tobytes()) + tuple(d[k].tobytes() for k in sorted(d))


def _run_case(oracle_mod, L, variants):
    from cetkmc import synthetic
    lat, calls = inputs(L)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    engines = {f: _engine(L, lat, f) for f in variants}
    logs = []
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(calls):
            kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, step0, n))
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            logs.append(ro)
            seen = {}
            for f, e in engines.items():
                rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                seen[f] = _observed(e, rg)
                assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"L={L} call {c}, fused_tiles {f}")
            for f in variants[1:]:
                for q, (x, y) in enumerate(zip(seen[variants[0]], seen[f])):
                    assert x == y, f"L={L} call {c}: item {q} of the observed state differs between fused_tiles {variants[0]} and {f}"
    finally:
        oracle_mod.set_threads(1)
    n_def = count_deferred(calls)
    assert n_def == sum(BATCHES) - len(BATCHES) - 2          # every step but each call's last and the one before each update
    for e in engines.values():
        cnt = e.counters()
        assert cnt["deferred_steps"] == n_def and cnt["incremental_steps"] == 0, cnt
        e.close()
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    cov = deferred_coverage(L, calls, logs, DEFECT_FRACTION)
    print(f"L={L} deferred-step coverage (oracle log): {cov}")
    assert min(cov["kinds"]) >= 1, cov                       # deposition, diffusion, nucleation, attachment: all on deferred steps
    return cov


def test_fused_tiles_L129(oracle_mod):
    """All three settings.  Oracle's log, 41 deferred steps: kinds [18, 5, 3, 15] (deposition, diffusion, nucleation, attachment),
    3 diffusions between planes, 4 defect injections."""
    _run_case(oracle_mod, 129, (1, 0, 2))


def test_fused_tiles_L160(oracle_mod):
    """Tiles renumbered per XCD (1600 tiles).  Oracle's log, 41 deferred steps: kinds [22, 4, 2, 13], 3 diffusions between planes."""
    from cetkmc import _lib
    lib = _lib.load()
    assert (lib.cetkmc_table_tile_of(160, 159, 159) + 1) % 8 == 0
    _run_case(oracle_mod, 160, (1, 0))


def test_fused_tiles_L256(oracle_mod):
    """The benchmark's size, 45 steps.  Oracle's log, 41 deferred steps: kinds [22, 3, 7, 9], one diffusion between planes."""
    _run_case(oracle_mod, 256, (1, 0))
