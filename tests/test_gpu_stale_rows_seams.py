"""Deferred steps whose stale rows straddle tile seams and lattice faces, at the smallest lattices that run that code.

A sweep launch that applies a pending event (k_sweep_stream_apply) stores each stale row once: the tiles whose 8 planes x 8
rows meet the 5 x 5 window of a site of the event leave those rows' stores out, the apply block re-evaluates and stores
them after the event.  Tile seams are at multiples of 8 in planes and rows; deferral needs 128 < L <= 256, so L = 129 is
the first lattice on the path and puts plane 128 and row 128 alone in a last, partial tile; L = 136 and 160 have none, and
L = 160 (20 x 20 tiles) takes the per-XCD block remapping ((number of tiles) % 8 == 0), which 17 x 17 tiles do not.

The lattice allows events only in seven small windows: everywhere else the empty voxels sit within delta_T_c of the melt (no
nucleation), plane L-1 is filled with inert atoms (no deposition), and W / Re / C atoms are placed only inside the windows.
The windows are centred on seams in i, in j, in both, on the faces and in the partial last tile.  thermal_mode 0: every
step but a call's last is deferred.  The run is compared with the immediate path bit for bit and with the oracle; what the
deferred steps exercised is counted from the ORACLE's log with the library's own enumeration of the stale rows."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import assert_call_matches_oracle, count_deferred, is_deferred, oracle_lattice, step_uniforms
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
TWEAK = dict(I0=1e12)          # nucleation beside diffusion and attachment in the cold windows
TILE = 8                       # STREAM_NI planes x SWEEP_TJ rows


def window_centres(L):
    return [(8, 8), (7, 16), (16, 9), (0, 0), (L - 1, L - 1), (L - 2, 64), (64, 0)]


def window_lattice(L, seed, half=1, k0=8, kn=24, t_cold=3600.0, n_atoms=10):
    """Empty lattice at T_melt - delta_T_c / 2, plane L-1 inert; per window ((2 half + 1)^2 rows, k0 <= k < k0 + kn): T =
    t_cold, n_atoms random W / Re / C atoms and, where the window reaches plane L-1, that plane empty at T_melt (deposition,
    no nucleation)."""
    import constants as K
    rs = np.random.RandomState(seed)
    st = np.zeros((L, L, L), np.uint8)
    th, ph = np.zeros((L, L, L)), np.zeros((L, L, L))
    df = np.zeros((L, L, L), np.uint8)
    T = np.full((L, L, L), K.T_MELT - 0.5 * K.DELTA_T_C)
    st[L - 1] = 4
    for (ci, cj) in window_centres(L):
        i0, i1 = max(ci - half, 0), min(ci + half, L - 1) + 1
        j0, j1 = max(cj - half, 0), min(cj + half, L - 1) + 1
        T[i0:i1, j0:j1, k0:k0 + kn] = t_cold
        if i1 == L:
            st[L - 1, j0:j1, k0:k0 + kn] = 0
            T[L - 1, j0:j1, k0:k0 + kn] = K.T_MELT
        for _ in range(n_atoms):
            i, j, k = rs.randint(i0, min(i1, L - 1)), rs.randint(j0, j1), rs.randint(k0, k0 + kn)
            st[i, j, k] = 1 + rs.randint(3)
            th[i, j, k], ph[i, j, k] = rs.uniform(0, np.pi), rs.uniform(0, 2 * np.pi)
    return st, th, ph, T, df


def make_calls(seed, batches):
    calls, s = [], 0
    for c, n in enumerate(batches):
        calls.append((s, n) + step_uniforms(300 + seed * 10 + c, n, 2 * n + 2))
        s += n
    return calls


def stale_rows(lib, ev, L):
    t = int(ev["type"])
    rows = (C.c_int * 64)()
    pos = (C.c_int * 2)(int(ev["pos"][0]), int(ev["pos"][1]))
    tgt = (C.c_int * 2)(int(ev["target"][0]), int(ev["target"][1])) if t == 1 else (C.c_int * 2)(0, 0)
    n = lib.cetkmc_stale_rows(t, pos, tgt, L, rows)
    return [(rows[2 * q], rows[2 * q + 1]) for q in range(n)]


def seam_coverage(L, calls, logs):
    """of the deferred steps of the oracle's logs: events by kind, events whose stale rows lie in two tiles along i / along
    j / in 2 x 2 tiles, events clipped at each face, diffusions whose two sites lie in different tiles"""
    from cetkmc import _lib
    lib = _lib.load()
    cov = dict(kinds=[0] * 4, two_i=0, two_j=0, four=0, face_i0=0, face_j0=0, face_i1=0, face_j1=0, diff_tiles=0)
    for (step0, n, *_), ro in zip(calls, logs):
        for x in range(ro["done"]):
            if not is_deferred(step0, n, x, 0):
                continue
            ev = ro["events"][x]
            t = int(ev["type"])
            rows = stale_rows(lib, ev, L)
            ti, tj = {r[0] // TILE for r in rows}, {r[1] // TILE for r in rows}
            sites = [ev["pos"]] + ([ev["target"]] if t == 1 else [])
            full = 11 * len(sites)        # rows of sites away from the faces (fewer also where two sites share rows)
            cov["kinds"][t] += 1
            cov["two_i"] += int(len(ti) == 2 and len(tj) == 1)
            cov["two_j"] += int(len(ti) == 1 and len(tj) == 2)
            cov["four"] += int(len(ti) == 2 and len(tj) == 2)
            cov["face_i0"] += int(len(rows) < full and any(s[0] < 2 for s in sites))
            cov["face_j0"] += int(len(rows) < full and any(s[1] < 2 for s in sites))
            cov["face_i1"] += int(len(rows) < full and any(s[0] > L - 3 for s in sites))
            cov["face_j1"] += int(len(rows) < full and any(s[1] > L - 3 for s in sites))
            cov["diff_tiles"] += int(t == 1 and (ev["pos"][0] // TILE, ev["pos"][1] // TILE) !=
                                     (ev["target"][0] // TILE, ev["target"][1] // TILE))
    return cov


def _engine(L, lat, on):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in TWEAK.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.set_option("apply_in_sweep", int(on))
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


def _observed(e, r):
    """Everything observable after a call.  What every sweep launch of the call stored -- tiles and apply block -- is in the
    logs: each step's total and event count are folded from that step's row sums, and its event is chosen from them.  The
    row sums themselves can be read only behind a plain sweep of the lattice the call left."""
    d = e.download(defects=True)
    info = e.rate_sweep()
    rs, rc = e.row_sums()
    return (r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["full_sweeps"], r["totals"].tobytes(),
            r["events"].tobytes(), r["n_events"].tobytes(), info, rs.tobytes(), rc.tobytes()) + tuple(d[k].tobytes() for k in sorted(d))


def _run_case(oracle_mod, L, seed, batches):
    lat = window_lattice(L, seed)
    calls = make_calls(seed, batches)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, TWEAK)
    on, off = _engine(L, lat, True), _engine(L, lat, False)
    logs = []
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(calls):
            kw = dict(rng_mode=1, seed=5, thermal_mode=0)
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            logs.append(ro)
            ra = on.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            rb = off.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            a, b = _observed(on, ra), _observed(off, rb)
            assert_call_matches_oracle(on, o, ra, ro, RATE_RTOL, tag=f"L={L} call {c}, apply_in_sweep on")
            assert a[:6] == b[:6], (c, a[:6], b[:6])
            for q, (x, y) in enumerate(zip(a, b)):
                assert x == y, f"L={L} call {c}: item {q} of the observed state differs between the deferred and the immediate path"
    finally:
        oracle_mod.set_threads(1)
    n_def = count_deferred(calls, thermal_mode=0)
    assert on.counters()["deferred_steps"] == n_def == sum(n - 1 for n in batches)
    assert off.counters()["deferred_steps"] == 0
    on.close()
    off.close()
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    cov = seam_coverage(L, calls, logs)
    print(f"L={L} deferred-step coverage (oracle log): {cov}")
    return cov


def _assert_coverage(cov):
    assert min(cov["kinds"]) >= 3, cov             # deposition, diffusion, nucleation, attachment
    for key in ("two_i", "two_j", "four", "face_i0", "face_j0", "face_i1", "face_j1", "diff_tiles"):
        assert cov[key] >= 1, (key, cov)


def test_seams_faces_and_partial_tile_L129(oracle_mod):
    """57 deferred steps in three calls.  The oracle's log for these inputs: kinds [16, 20, 10, 11]; stale rows in two tiles
    along i 8 times, along j twice, in four tiles 41 times; clipped at i = 0 / j = 0 / i = L-1 / j = L-1 5 / 9 / 22 / 12
    times; 5 diffusions between tiles."""
    cov = _run_case(oracle_mod, 129, 2, (25, 20, 15))
    _assert_coverage(cov)


@pytest.mark.parametrize("L", [136, 160])
def test_seams_without_partial_tile(oracle_mod, L):
    """A shorter run (21 deferred steps in two calls) at multiples of 8, where no tile is partial.  The tiles of a launch
    are renumbered into contiguous ranges per XCD when their number is a multiple of 8: 17 x 17 tiles at L = 136 are not
    (natural order), 20 x 20 at L = 160 are, so the window test runs on the remapped tile index too.  The oracle's log
    gives kinds [10, 4, 4, 3] at both sizes and every seam / face count >= 1."""
    n_tiles = ((L + TILE - 1) // TILE) ** 2
    assert (n_tiles % 8 == 0) == (L == 160)
    cov = _run_case(oracle_mod, L, 3, (14, 9))
    _assert_coverage(cov)
