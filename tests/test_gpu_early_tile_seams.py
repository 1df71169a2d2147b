"""Option early_tiles: events steered into windows around the seam between the last early tile and the first late one.

A deferred step's selection launch runs the tiles [0, E) of the next step's sweep into the other row-sum pair, the sweep launch
behind it the tiles [E, count) and, in its apply block, the rows the event makes stale.  Around the seam an event's stale
rows lie partly in rows an early tile has already stored (from the lattice before the event: the apply block must overwrite
them) and partly in rows a late tile leaves out; a diffusion can have its site on one side and its target on the other.

The method and the lattice are those of test_gpu_fused_tile_seams.py (events only in small cold windows, thermal_mode 0, every
step but a call's last deferred), with the windows centred where the seams of three values of E lie, one engine per value:
  interior  E = the tile that begins inside plane 40; window on its first row;
  face      E = a tile that begins with row 0 of a plane p; windows at (p, 0) and (p - 1, L - 1);
  top       E = a tile that begins inside plane L - 1; window on its first row (deposition in plane L - 1).
Each engine runs with poison_alt_rows = 1 and is compared with early_tiles = 0 bit for bit and with the oracle.  The coverage is
counted from the ORACLE's log with the library's own stale-row enumeration and cetkmc_early_tile_row(); the seeds were chosen
with the oracle alone on the CPU so that every class is hit (counts in the test's docstring)."""
import os

import pytest

from helpers import assert_call_matches_oracle, count_deferred, is_deferred, oracle_lattice
from test_gpu_early_tiles import frozen
from test_gpu_fused_tile_seams import _observed, _tile, seam_row, window_lattice
from test_gpu_parity import RATE_RTOL
from test_gpu_stale_rows_seams import DEFECT_FRACTION, IMPURITY_C, TWEAK, make_calls, stale_rows

pytestmark = pytest.mark.gpu


def first_row(L, E):
    """(plane, row) of the first row of tile E"""
    ipp = (L + 1) // 2
    return 8 * E // ipp, 2 * (8 * E % ipp)


def seams(lib, L):
    """{class: (E, window centres)}"""
    ipp = (L + 1) // 2
    e_int = _tile(lib, L, 40, seam_row(lib, L, 40))
    e_face = next(E for E in range(8 * ipp // 8, 10 ** 6) if 8 * E % ipp == 0 and 8 * E // ipp >= 20)
    e_top = _tile(lib, L, L - 1, seam_row(lib, L, L - 1))
    p = first_row(L, e_face)[0]
    assert first_row(L, e_int)[0] == 40 and first_row(L, e_face) == (p, 0) and first_row(L, e_top)[0] == L - 1
    return {"interior": (e_int, [first_row(L, e_int)]), "face": (e_face, [(p, 0), (p - 1, L - 1)]), "top": (e_top, [first_row(L, e_top)])}


def inputs(lib, L, seed, batches):
    centres = [c for (_, cs) in seams(lib, L).values() for c in cs]
    return window_lattice(L, centres, seed), make_calls(seed, batches)


def seam_coverage(lib, L, E, calls, logs):
    """Of the deferred steps of the oracle's logs, for early_tiles = E: events whose stale rows lie on both sides (split), those
    among them with a site at j <= 1 or j >= L - 2 (split_face) or in plane L - 1 (split_top), diffusions whose site and target
    lie on different sides (diff_across), and the events by kind."""
    cov = dict(kinds=[0] * 4, split=0, split_face=0, split_top=0, diff_across=0)
    side = lambda gi, j: lib.cetkmc_early_tile_row(L, E, int(gi), int(j))
    for (step0, n, *_), ro in zip(calls, logs):
        for x in range(ro["done"]):
            if not is_deferred(step0, n, x, 0):
                continue
            ev = ro["events"][x]
            t = int(ev["type"])
            sites = [ev["pos"]] + ([ev["target"]] if t == 1 else [])
            split = {side(gi, j) for (gi, j) in stale_rows(lib, ev, L)} == {0, 1}
            cov["kinds"][t] += 1
            cov["split"] += int(split)
            cov["split_face"] += int(split and any(s[1] <= 1 or s[1] >= L - 2 for s in sites))
            cov["split_top"] += int(split and any(s[0] == L - 1 for s in sites))
            cov["diff_across"] += int(t == 1 and side(*ev["pos"][:2]) != side(*ev["target"][:2]))
    return cov


def assert_coverage(covs):
    assert covs["interior"]["split"] >= 1 and covs["interior"]["diff_across"] >= 1, covs["interior"]
    assert covs["face"]["split_face"] >= 1 and covs["face"]["diff_across"] >= 1, covs["face"]
    assert covs["top"]["split_top"] >= 1 and covs["top"]["diff_across"] >= 1, covs["top"]
    assert min(min(c["kinds"]) for c in covs.values()) >= 1, covs


def _engine(L, lat, early):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in TWEAK.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.set_option("early_tiles", early)
    e.set_option("poison_alt_rows", 1 if early else 0)
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


CASES = {129: (10, (25, 20, 15)), 136: (18, (22, 14))}      # L: (seed, steps per call)


@pytest.mark.parametrize("L", sorted(CASES))
def test_early_tile_seams(oracle_mod, L):
    """L = 129 (seed 10, 57 deferred steps in three calls): E = 326 at (40, 16), 195 at (24, 0) / (23, 128), 1041 at (128, 16).  The
    oracle's log for these inputs (checked on the CPU with the oracle alone): kinds [19, 17, 6, 15]; interior: 12 events with
    stale rows on both sides, 1 diffusion across; face: 12 split, 10 of them with a site on a j face, 1 diffusion across; top: 31
    split, 23 of them with a site in plane L - 1, 1 diffusion across.  L = 136 (seed 18, 34 deferred steps in two calls): E =
    341 at (40, 16), 170 at (20, 0) / (19, 135), 1148 at (135, 8); kinds [9, 13, 2, 10]; interior 5 split, 1 diffusion across;
    face 12 / 11 / 1; top 15 / 14 / 1."""
    from cetkmc import _lib
    lib = _lib.load()
    seed, batches = CASES[L]
    lat, calls = inputs(lib, L, seed, batches)
    sm = seams(lib, L)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, TWEAK)
    engines = {0: _engine(L, lat, 0)}
    engines.update({E: _engine(L, lat, E) for (E, _) in sm.values()})
    logs = []
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(calls):
            kw = dict(rng_mode=1, seed=5, thermal_mode=0)
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            logs.append(ro)
            left = frozen(o)
            seen = {}
            for E, e in engines.items():
                rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                seen[E] = _observed(e, rg)
                assert_call_matches_oracle(e, left, rg, ro, RATE_RTOL, tag=f"L={L} call {c}, early_tiles {E}")
            for E in engines:
                for q, (x, y) in enumerate(zip(seen[0], seen[E])):
                    assert x == y, f"L={L} call {c}: item {q} of the observed state differs between early_tiles 0 and {E}"
    finally:
        oracle_mod.set_threads(1)
    n_def = count_deferred(calls, thermal_mode=0)
    for E, e in engines.items():
        cnt = e.counters()
        assert cnt["deferred_steps"] == n_def == sum(n - 1 for n in batches) and cnt["early_tiles"] == n_def * E, (E, cnt)
        e.close()
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    covs = {name: seam_coverage(lib, L, E, calls, logs) for name, (E, _) in sm.items()}
    print(f"L={L} seams {sm}\ndeferred-step coverage (oracle log): {covs}")
    assert_coverage(covs)
