"""Option early_tiles: a deferred step's selection launch (k_select_pend_tiles) runs the first E tiles of the next step's sweep,
the next sweep launch (k_sweep_stream_apply) the remaining ones, against early_tiles = 0 bit for bit and against the oracle.

The early tiles store into the handle's second pair of row-sum buffers, which then becomes the current pair; the late tiles,
the apply block's stale rows, the reduce and the next selection use that pair.  Every engine with E > 0 runs with
poison_alt_rows = 1: the pair a deferred step is about to write is filled with 0xFF bytes first, so a row that neither an early
tile nor a late tile nor the apply block stores is a NaN in that step's total and a wrong count in its block.

E per lattice, one block per tile (early_blocks = 0): 1 and 8 (a launch of one tile; of eight, the smallest that is renumbered
per XCD), a multiple of 8 near the middle (both launches renumbered), count - 1 (one late tile), count (the sweep launch is the
apply block alone) and count + 5 (clipped to count).  Then in fewer blocks than tiles (option early_blocks): 24 blocks that loop
over half the tiles and 7 over all of them.  The L = 256 case runs the library's defaults (a quarter of the tiles in 256
blocks).  Lattices as test_gpu_lane_skip (kfill = 34; L = 129 odd, so the last row pair of a plane is half empty, 1049 tiles;
136: 1156; 160: 1600, a multiple of 8).  45 steps from step 0 in two calls on one handle: temperature updates at steps 20 and
40, the immediate step before each, each call's last (immediate) step, and the parity of the pairs across the call boundary.

The oracle runs each call once; its sweep of the lattice the call left is shared by the engines."""
import os
import types

import pytest

from helpers import (FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, count_deferred, deferred_coverage, face_lattice,
                     oracle_lattice)
from test_gpu_lane_skip import KFILL, N_ATOMS, lattice
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
BATCHES = (24, 21)                 # steps 0..44: temperature updates at steps 20 and 40, one inside each call
DEFAULT_EARLY = 1024               # the library's default of early_tiles at L = 256: a quarter of its 4096 tiles


def tile_count(L):
    return ((L + 1) // 2 * L + 7) // 8


def early_values(L):
    n = tile_count(L)
    return (1, 8, 8 * (n // 16), n - 1, n, n + 5, (8 * (n // 16), 24), (n, 7))


def _engine(L, lat, early):
    """early None: the library's defaults, untouched; (E, G): early_tiles = E in early_blocks = G blocks"""
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    if early is None:
        e.set_option("poison_alt_rows", 1)
    else:
        E, G = early if isinstance(early, tuple) else (early, 0)
        e.set_option("early_tiles", E)
        e.set_option("early_blocks", G)
        e.set_option("poison_alt_rows", 1 if E else 0)
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


def _observed(e, r):
    """the event log, the totals, the candidate counts, the stream positions and the final fields of a call"""
    d = e.download(defects=True)
    return (r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["full_sweeps"], r["totals"].tobytes(),
            r["events"].tobytes(), r["n_events"].tobytes()) + tuple(d[k].tobytes() for k in sorted(d))


def frozen(o):
    """the oracle lattice as a call left it, with ONE sweep of it for every engine that is compared against it"""
    sw = o.sweep()
    return types.SimpleNamespace(state=o.state, theta=o.theta, phi=o.phi, T=o.T, defects=o.defects, nuc_count=o.nuc_count,
                                 sweep=lambda: sw)


def _run_case(oracle_mod, L, lat, variants):
    """variants: values of early_tiles, the first one the reference the others are compared with bit for bit"""
    from cetkmc import synthetic
    calls = batch_calls(BATCHES)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    engines = {v: _engine(L, lat, v) for v in variants}
    logs = []
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(calls):
            kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, step0, n))
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            logs.append(ro)
            left = frozen(o)
            seen = {}
            for v, e in engines.items():
                rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                seen[v] = _observed(e, rg)
                assert_call_matches_oracle(e, left, rg, ro, RATE_RTOL, tag=f"L={L} call {c}, early_tiles {v}")
            for v in variants[1:]:
                for q, (x, y) in enumerate(zip(seen[variants[0]], seen[v])):
                    assert x == y, f"L={L} call {c}: item {q} of the observed state differs between early_tiles {variants[0]} and {v}"
    finally:
        oracle_mod.set_threads(1)
    n_def = count_deferred(calls)
    assert n_def == sum(BATCHES) - len(BATCHES) - 2          # every step but each call's last and the one before each update
    ref = engines[variants[0]].counters()
    for v, e in engines.items():
        cnt = e.counters()
        want = DEFAULT_EARLY if v is None else v[0] if isinstance(v, tuple) else v
        assert cnt["deferred_steps"] == ref["deferred_steps"] == n_def and cnt["incremental_steps"] == 0, (v, cnt)
        assert cnt["early_tiles"] == n_def * min(want, tile_count(L)), (v, cnt["early_tiles"])
        assert cnt["sweeps"] == ref["sweeps"] and cnt["interface_launches"] == ref["interface_launches"], (v, cnt)
        e.close()
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    cov = deferred_coverage(L, calls, logs, DEFECT_FRACTION)
    print(f"L={L} deferred-step coverage (oracle log): {cov}")
    assert min(cov["kinds"]) >= 1, cov                       # deposition, diffusion, nucleation, attachment: all on deferred steps
    return cov


@pytest.mark.parametrize("L", [129, 136, 160])
def test_early_tiles(oracle_mod, L):
    """kfill = 34 lattices of test_gpu_lane_skip.  Oracle's log, 41 deferred steps, all four kinds at every size (printed)."""
    assert KFILL == 34 and N_ATOMS == 6000
    _run_case(oracle_mod, L, lattice(L, 17 + L, False), (0,) + early_values(L))


def test_early_tiles_L256_default(oracle_mod):
    """The benchmark's size with the library's defaults against early_tiles = 0 (test_gpu_fused_tiles' lattice)."""
    _run_case(oracle_mod, 256, face_lattice(256, 17 + 256, 24000), (0, None))
