"""Option lane_sweep: a plain sweep launch on a fresh lane table runs the lane-sum tiles of the deferred launches over the full
tile range (k_sweep_stream<.., LU>), against the plain launch that reads every entry (lane_sweep 0), against the building sweep
of the same lattice, bit for bit through cetkmc_row_sums, and against the oracle.

L = 129: odd, the last row has no partner in its half-wave pair and the row's last chunk is padded; L = 136: 17 whole chunks.
The first rate_sweep() of an uploaded lattice builds the lane table (k_rate_table wrote the rate table: the temperature tiles
that could build it run at L = 256 only); every plain launch after it finds the table fresh: a second rate_sweep(), the
immediate steps of a stepping call -- the last step of every call, every step of a one-step call -- and the sweep after it, by
then with the chunks poisoned that the events wrote into."""
import os

import numpy as np
import pytest

from helpers import FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, oracle_lattice, relerr
from test_gpu_lane_sums import DEFECT_FRACTION, IMPURITY_C, _engine, ramp_lattice
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

BATCHES = (7, 1, 4)        # from step 1: no temperature update; six deferred steps, then calls of one and four steps


def _sweep(e):
    tot = e.rate_sweep()
    rsum, rcnt = e.row_sums()
    return tot, rsum.copy(), rcnt.copy()


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert np.array_equal(a[1].view(np.int64), b[1].view(np.int64)), (what, "row sums", np.argwhere(a[1].view(np.int64) != b[1].view(np.int64))[:4])
    assert np.array_equal(a[2], b[2]), (what, "row counts", np.argwhere(a[2] != b[2])[:4])


def _against_oracle(o, s, what):
    sw = o.sweep()
    assert s[0][1:] == (sw["n_events"], sw["n_dep"]), (what, s[0], sw["n_events"], sw["n_dep"])
    assert np.array_equal(s[2], sw["rowcnt"]), (what, "rowcnt")
    assert relerr(s[1], sw["rowsum"]).max() <= RATE_RTOL and abs(s[0][0] - sw["total"]) <= RATE_RTOL * sw["total"], what


@pytest.mark.parametrize("L", [129, 136])
def test_plain_launch_reads_lane_sums(oracle_mod, L):
    lat = ramp_lattice(L)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    engines = {}
    for ls in (1, 0):
        e = engines[ls] = _engine(L, lat, 1, FOUR_KIND_PARAMS)
        e.set_option("lane_sweep", ls)
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        built = {ls: _sweep(e) for ls, e in engines.items()}          # the building sweep
        for ls, e in engines.items():
            t = e.lane_table()
            assert (t["fresh"], t["builds"], t["builds_thermal"]) == (1, 1, 0) and 2 * t["usable"] >= t["chunks"], (ls, t)
        t_built = engines[1].lane_table()
        fresh = {ls: _sweep(e) for ls, e in engines.items()}          # a plain launch on the fresh table
        _same(built[1], built[0], "building sweeps")
        _same(fresh[1], built[1], "lane-sum launch against the building sweep")
        _same(fresh[0], built[1], "lane_sweep 0 against the building sweep")
        _against_oracle(o, fresh[1], "fresh table")
        for c, (step0, n, u_pick, u_def, u_np) in enumerate(batch_calls(BATCHES, step0=1)):
            from cetkmc import synthetic
            kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, step0, n))
            ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
            assert (ro["done"], ro["status"]) == (n, 0)
            after = {}
            for ls, e in engines.items():
                rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"L={L} call {c}, lane_sweep {ls}")
                after[ls] = _sweep(e) + (rg["totals"].tobytes(), rg["events"].tobytes())
            _same(after[1], after[0], f"call {c}: sweep of the lattice it left")
            assert after[1][3:] == after[0][3:], f"call {c}: totals or event log differ between lane_sweep 1 and 0"
            _against_oracle(o, after[1], f"call {c}")
        for ls, e in engines.items():
            t = e.lane_table()
            # no plain launch rebuilt; the events poisoned chunks, and the launches above ran over them
            assert (t["fresh"], t["builds"]) == (1, 1) and t["poisoned"] > t_built["poisoned"], (ls, t, t_built)
            e.close()
    finally:
        oracle_mod.set_threads(1)
