"""cetkmc_remelt (one pass, now) against the comparator tests/remelt_ref.py at L = 1, 2, 3, 5, 33, 64, 65, 129 and 264.

Molten sets (tests/remelt_cases.direct_case; tests/test_remelt_ref_host.py checks on the comparator alone that they hold what
they claim): "crafted" = the eight corners, an edge, a face centre, an interior voxel, k-runs across 7/8/9 and 63/64/65 and a
row's last voxel, T exactly on the threshold, one ulp below it, NaN, +inf, and empty voxels above the threshold whose
orientation is kept; a whole plane; the whole lattice; nothing.  After the pass: the five fields, info, cetkmc_rate_sweep
(total within 1e-11 relative, counts ==), cetkmc_row_sums, cetkmc_enumerate_events at L <= 16; a second pass melts nothing;
prev_state through its effect (a nucleation applied onto a melted voxel releases latent heat at the next laser update); then
25 Mode A steps against the oracle, for every molten set.  For the plane, whole-lattice and nothing sets the rate table is
fresh when the pass runs (a sweep precedes it), for the crafted set it is first written after the pass."""
import numpy as np
import pytest

import remelt_cases as rc
from helpers import assert_call_matches_oracle, assert_fields_match_oracle, relerr, step_uniforms
from remelt_ref import remelt
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


def _events_match(e, lat):
    ev_o, _ = lat.enumerate()
    ev_g, n_g = e.enumerate_events()
    assert n_g == len(ev_o)
    for f in ("type", "pos", "target", "atom"):
        assert np.array_equal(ev_g[f], ev_o[f]), f
    if len(ev_o):
        assert relerr(ev_g["rate"], ev_o["rate"]).max() <= RATE_RTOL


@pytest.mark.parametrize("kind", rc.DIRECT_KINDS)
@pytest.mark.parametrize("L", rc.DIRECT_SIZES)
def test_one_pass_vs_comparator(oracle_mod, L, kind):
    import cetkmc
    fields, thr, claim = rc.direct_case(L, kind)
    oracle_mod.set_threads(16 if L > 100 else 1)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        e.upload(*fields)
        lat = oracle_mod.Lattice(*fields, impurity_c=IMPURITY_C)
        state0 = lat.state.copy()
        assert e.remelt_info() == dict(passes=0, n_melted=0, n_melted_last=0, n_appended=0)
        if kind != "crafted":
            # the rate table is written BEFORE the pass: in "plane" and "all" most melted voxels are neither listed nor appended
            # (their neighbours melt too), and the sweeps below read their entries as this table left them
            e.rate_sweep()
        info = e.remelt(thr)
        k = remelt(lat, thr)
        assert k >= len(claim["melts"]) and (kind != "nothing" or k == 0)
        assert (info["passes"], info["n_melted"], info["n_melted_last"]) == (1, k, k), (info, k)
        assert 0 <= info["n_appended"] <= L ** 3 and (k > 0 or info["n_appended"] == 0)
        assert e.remelt_info() == info
        assert_fields_match_oracle(e, lat, RATE_RTOL, f"L={L} {kind}")
        if L <= 16:
            _events_match(e, lat)
        # a second pass melts nothing and appends nothing
        info2 = e.remelt(thr)
        assert info2 == dict(info, passes=2, n_melted_last=0), (info, info2)
        assert_fields_match_oracle(e, lat, RATE_RTOL, f"L={L} {kind}, second pass")
        # prev_state == 0 on a melted voxel: an atom nucleated there releases latent heat at the next update
        gone = np.argwhere((state0 != 0) & (lat.state == 0))
        if len(gone):
            v = tuple(int(x) for x in gone[len(gone) // 2])
            ev_g, ev_o = cetkmc.Event(), oracle_mod.Event()
            for ev in (ev_g, ev_o):
                ev.type, ev.atom, ev.rate, ev.dep_rank = 2, 1, 1.0, -1
                ev.pos[:] = v
                ev.target[:] = (-1, -1, -1)
            e.apply(ev_g, 0.7, 1.9)
            lat.apply(ev_o, 0.7, 1.9)
            q = rc.scan_planes(L, 1)[0]
            e.thermal_laser(1e-6, q, use_latent=True, scrub_nan=True)
            released = lat.prev_state[v] == 0 and lat.state[v] != 0
            lat.thermal_laser(1e-6, q, scrub_nan=True)
            assert released
            assert np.array_equal(e.download()["T"], lat.T, equal_nan=True)
        n = 25
        u_pick, u_def, u_np = step_uniforms(3 + L, n, 2 * n + 2)
        rg = e.run_steps(1, n, 0.05, u_pick, u_def, u_np, rng_mode=1, seed=7, thermal_mode=1)
        ro = lat.run_steps(1, n, 0.05, u_pick, u_def, u_np, rng_mode=1, seed=7, thermal_mode=1)
        assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, f"L={L} {kind}, 25 steps")
        assert e.remelt_info() == info2               # remelting is off in the loop: the steps run no pass
    finally:
        e.close()
        oracle_mod.set_threads(1)


def test_replica_handle_and_counts_accumulate(oracle_mod):
    """the direct pass on a replica of an ensemble, and running totals over passes with different thresholds"""
    import cetkmc
    L = 33
    fields, thr, _ = rc.direct_case(L, "crafted")
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(2)])
    try:
        for r in range(2):
            ens.replica(r).upload(*fields)
        lat = oracle_mod.Lattice(*fields, impurity_c=IMPURITY_C)
        e = ens.replica(1)
        k1 = remelt(lat, thr)
        i1 = e.remelt(thr)
        k2 = remelt(lat, 3400.0)
        i2 = e.remelt(3400.0)
        assert k1 > 0 and k2 > 0
        assert (i1["passes"], i1["n_melted"], i1["n_melted_last"]) == (1, k1, k1)
        assert (i2["passes"], i2["n_melted"], i2["n_melted_last"]) == (2, k1 + k2, k2) and i2["n_appended"] >= i1["n_appended"]
        assert_fields_match_oracle(e, lat, RATE_RTOL, "replica 1")
        untouched = oracle_mod.Lattice(*fields, impurity_c=IMPURITY_C)
        assert_fields_match_oracle(ens.replica(0), untouched, RATE_RTOL, "replica 0")
        assert ens.remelt_info() == [dict(passes=0, n_melted=0, n_melted_last=0, n_appended=0), i2]
    finally:
        ens.close()
