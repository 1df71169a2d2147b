"""Deferred steps whose stale rows meet the seams of the census-free tiles (option fused_tiles), at the smallest lattices
that run them.

With fused_tiles on, the tiles of the sweep launch that applies a pending event (k_sweep_stream_apply) own consecutive ranges
of items -- item = plane * ((L + 1) / 2) + row pair, cetkmc_table_tile_of() -- and every tile tests each row it is about to
store against the record (stale_row()); the apply block stores the stale rows.  The seams of that decomposition are not
those of the ring tiles (multiples of 8 in planes and rows): a tile's range ends in the middle of a plane, at another row in
every plane, and mostly runs on from the last row pairs of one plane into the first of the next; rows 2p and 2p + 1 share a
wave; at odd L the last row has no partner.  L = 129 is the first lattice on the path (65 pairs per plane, the last one
half empty); L = 136 has 68 pairs per plane.

The method is that of test_gpu_stale_rows_seams.py: events can happen only in small windows (everywhere else the empty
voxels sit within delta_T_c of the melt, plane L-1 is inert, impurities only inside the windows), thermal_mode 0, so that
every step but a call's last is deferred.  The window centres are taken from the mapping the library ships: on a seam inside
a plane, at both ends of a tile range that wraps between planes, on the faces.  fused_tiles 1 is compared with fused_tiles 0
bit for bit and with the oracle; what the deferred steps exercised is counted from the ORACLE's log with the library's own
enumeration of the stale rows and its own tile mapping, and every class must have been hit."""
import os

import numpy as np
import pytest

from helpers import assert_call_matches_oracle, count_deferred, is_deferred, oracle_lattice
from test_gpu_parity import RATE_RTOL
from test_gpu_stale_rows_seams import DEFECT_FRACTION, IMPURITY_C, TWEAK, make_calls, stale_rows

pytestmark = pytest.mark.gpu


def _tile(lib, L, gi, j):
    t = lib.cetkmc_table_tile_of(L, int(gi), int(j))
    assert t >= 0, (L, gi, j)
    return t


def seam_row(lib, L, gi):
    """the first row >= 4 of plane gi that begins another tile than the row before it"""
    return next(j for j in range(4, L - 4) if _tile(lib, L, gi, j) != _tile(lib, L, gi, j - 1))


def wrap_plane(lib, L, lo):
    """the first plane >= lo whose first row lies in the tile that owns the last row of the plane before"""
    return next(p for p in range(lo, L - 3) if _tile(lib, L, p, 0) == _tile(lib, L, p - 1, L - 1))


def window_centres(lib, L):
    p0, p1 = wrap_plane(lib, L, 40), wrap_plane(lib, L, 70)
    return [(8, seam_row(lib, L, 8)), (17, seam_row(lib, L, 17) + 1),       # a seam inside a plane, two positions against the pairs
            (p0, 0), (p1 - 1, L - 1),                                        # head and tail of a range that wraps between planes
            (0, 0), (L - 1, L - 1), (L - 2, 64), (64, 0)]                    # faces (and deposition in plane L-1)


def window_lattice(L, centres, seed, half=1, k0=8, kn=24, t_cold=3600.0, n_atoms=10):
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
    for (ci, cj) in centres:
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


def inputs(lib, L, seed, batches):
    return window_lattice(L, window_centres(lib, L), seed), make_calls(seed, batches)


def seam_coverage(lib, L, calls, logs):
    """Of the deferred steps of the oracle's logs: events by kind; events whose stale rows OF ONE PLANE lie in two tiles
    (straddle); events at j >= L-2 / j <= 1 with a stale row in a tile that owns rows of two planes, in its earlier / later
    plane (wrap_tail / wrap_head); events with a row pair of which one row only is stale (half_pair); events that make the
    partnerless last row of an odd L stale (lone_row); events clipped at each face; diffusions between two tiles."""
    cov = dict(kinds=[0] * 4, straddle=0, wrap_tail=0, wrap_head=0, half_pair=0, lone_row=0, face_i0=0, face_j0=0, face_i1=0,
               face_j1=0, diff_tiles=0)
    two_planes = lambda gi, j, d: 0 <= gi + d < L and _tile(lib, L, gi, j) == _tile(lib, L, gi + d, 0 if d > 0 else L - 1)
    for (step0, n, *_), ro in zip(calls, logs):
        for x in range(ro["done"]):
            if not is_deferred(step0, n, x, 0):
                continue
            ev = ro["events"][x]
            t = int(ev["type"])
            rows = set(stale_rows(lib, ev, L))
            sites = [ev["pos"]] + ([ev["target"]] if t == 1 else [])
            full = 11 * len(sites)        # rows of sites away from the faces (fewer also where two sites share rows)
            cov["kinds"][t] += 1
            cov["straddle"] += int(any(len({_tile(lib, L, gi, j) for (gi, j) in rows if gi == p}) > 1 for p in {r[0] for r in rows}))
            cov["wrap_tail"] += int(any(s[1] >= L - 2 for s in sites) and any(two_planes(gi, j, +1) for (gi, j) in rows))
            cov["wrap_head"] += int(any(s[1] <= 1 for s in sites) and any(two_planes(gi, j, -1) for (gi, j) in rows))
            cov["half_pair"] += int(any(((gi, j ^ 1) not in rows) and (j ^ 1) < L for (gi, j) in rows))
            cov["lone_row"] += int(L % 2 == 1 and any(j == L - 1 for (_, j) in rows))
            cov["face_i0"] += int(len(rows) < full and any(s[0] < 2 for s in sites))
            cov["face_j0"] += int(len(rows) < full and any(s[1] < 2 for s in sites))
            cov["face_i1"] += int(len(rows) < full and any(s[0] > L - 3 for s in sites))
            cov["face_j1"] += int(len(rows) < full and any(s[1] > L - 3 for s in sites))
            cov["diff_tiles"] += int(t == 1 and _tile(lib, L, ev["pos"][0], ev["pos"][1]) != _tile(lib, L, ev["target"][0], ev["target"][1]))
    return cov


def assert_coverage(L, cov):
    assert min(cov["kinds"]) >= 1, cov             # deposition, diffusion, nucleation, attachment
    for key in ("straddle", "wrap_tail", "wrap_head", "half_pair", "face_i0", "face_j0", "face_i1", "face_j1", "diff_tiles"):
        assert cov[key] >= 1, (key, cov)
    assert L % 2 == 0 or cov["lone_row"] >= 1, cov


def _engine(L, lat, fused):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in TWEAK.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.set_option("fused_tiles", fused)
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


def _observed(e, r):
    """Everything observable after a call.  What every sweep launch of the call stored -- tiles and apply block -- is in the
    logs: each step's total and event count are folded from that step's row sums, and its event is chosen from them."""
    d = e.download(defects=True)
    info = e.rate_sweep()
    rs, rc = e.row_sums()
    return (r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["full_sweeps"], r["totals"].tobytes(),
            r["events"].tobytes(), r["n_events"].tobytes(), info, rs.tobytes(), rc.tobytes()) + tuple(d[k].tobytes() for k in sorted(d))


CASES = {129: (2, (25, 20, 15)), 136: (3, (22, 14))}


@pytest.mark.parametrize("L", sorted(CASES))
def test_table_tile_seams(oracle_mod, L):
    """L = 129: 57 deferred steps in three calls; the oracle's log for these inputs (checked on the CPU with the oracle alone)
    gives kinds [16, 16, 10, 15], straddle 41, wrap_tail 16, wrap_head 13, half_pair 57, lone_row 17, faces i0 / j0 / i1 / j1
    4 / 13 / 20 / 16, diff_tiles 13; window centres (8, 16), (17, 15), (41, 0), (69, 128) + faces (tiles of 8 items).  L = 136:
    34 deferred steps in two calls; kinds [11, 14, 4, 5], straddle 13, wrap_tail 10, wrap_head 5, half_pair 34, faces
    1 / 5 / 15 / 10, diff_tiles 8; centres (8, 16), (17, 9), (41, 0), (70, 135) + faces."""
    from cetkmc import _lib
    lib = _lib.load()
    seed, batches = CASES[L]
    lat, calls = inputs(lib, L, seed, batches)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, TWEAK)
    on, off = _engine(L, lat, 1), _engine(L, lat, 0)
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
            assert_call_matches_oracle(on, o, ra, ro, RATE_RTOL, tag=f"L={L} call {c}, fused_tiles 1")
            for q, (x, y) in enumerate(zip(a, b)):
                assert x == y, f"L={L} call {c}: item {q} of the observed state differs between fused_tiles 1 and 0"
    finally:
        oracle_mod.set_threads(1)
    n_def = count_deferred(calls, thermal_mode=0)
    assert on.counters()["deferred_steps"] == off.counters()["deferred_steps"] == n_def == sum(n - 1 for n in batches)
    on.close()
    off.close()
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, calls))
    cov = seam_coverage(lib, L, calls, logs)
    print(f"L={L} deferred-step coverage (oracle log): {cov}")
    assert_coverage(L, cov)
