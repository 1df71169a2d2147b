"""Beam tables in replica ensembles (cetkmc_ensemble_set_beam + cetkmc_run_ensemble with thermal_mode 2 and no plane sets): every
replica against the comparator tests/beam_ref.py after every call, L = 30 (R = 3, one table per replica, reference streams,
n = 1, depth 2) and L = 33 (R = 70, two tables through set_of, counter-based uniforms, n = 3, depth 3), a replica that terminates
in the first call and is frozen in the second, an empty replica; and a replica's bytes against a single handle's with the same
table."""
import numpy as np
import pytest

import beam_cases as bm
import implicit_cases as ic
import remelt_cases as rc
from helpers import assert_ensemble_call_matches_oracle
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


@pytest.mark.parametrize("name,R,n_sets", [("ens_L30_n1_D2", 3, 3), ("ens_L33_n3_D3", 70, 2)])
def test_every_replica_vs_comparator(oracle_mod, name, R, n_sets):
    import cetkmc
    case, runs = bm.replica_runs(name, R, n_sets)
    L, n_calls, n_sub = case["L"], len(case["batches"]), case["n_sub"]
    assert runs[0][0]["results"][0]["status"] == 1 and runs[0][0]["results"][0]["done"] == 0      # terminates, then frozen
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(R)])
    try:
        for r, (run, _) in enumerate(runs):
            ens.replica(r).upload(*run["lat0"])
        ens.set_thermal_substeps(n_sub)
        ens.set_thermal_scheme("implicit")
        tables = [bm.table_of(case, p) for p in bm.ENS_POWERS[:n_sets]]
        set_of = [s for _, s in runs]
        assert len(set(set_of)) == n_sets
        ens.set_beam(tables, None if set_of == list(range(R)) else set_of)
        updates = 0
        for c in range(n_calls):
            calls = [run["calls"][c] for run, _ in runs]
            s0, n = calls[0][0], calls[0][1]
            kw = dict(thermal_mode=2, use_latent=case["use_latent"])
            if case["rng_mode"] == 0:
                res = ens.run(s0, n, case["defect_fraction"], np.stack([x[2] for x in calls]), np.stack([x[3] for x in calls]),
                              np.stack([x[4] for x in calls]), rng_mode=0, **kw)
            else:
                seeds = [case["seed"]] * 2 + [case["seed"] + r % 3 for r in range(2, R)]
                res = ens.run(s0, n, case["defect_fraction"], rng_mode=2, seeds=seeds, **kw)
            lats, ros = [], []
            for r, (run, _) in enumerate(runs):
                done_before = len(run["results"]) <= c          # the comparator stopped stepping it: frozen in this call
                cc = min(c, len(run["results"]) - 1)
                lats.append(rc.LatView(run, cc, IMPURITY_C))
                ros.append(None if done_before else run["results"][c])
            assert_ensemble_call_matches_oracle(ens, lats, res, ros, RATE_RTOL, f"{name} call {c}")
            updates += updates_in(s0, n)
            assert ens.beam_info() == dict(updates=updates, steps=updates * n_sub, launches=3 * updates * n_sub, table_uploads=1)
            assert ens.implicit_info()["updates"] == updates
        assert updates >= 2
    finally:
        ens.close()


def test_replica_bytes_equal_a_single_handle(oracle_mod):
    """the same lattice, calls, seed and table on a single handle and as replica 1 of three (which reads set 1 of two), n = 3; then
    one direct update on the replica's handle from the ensemble's table"""
    import cetkmc
    case = bm.ENSEMBLE["ens_L33_n3_D3"]
    L = case["L"]
    lat0 = ic.lattice_of(case)
    calls = bm.calls_of(case)
    ta, tb = bm.table_of(case, 1.0), bm.table_of(case, 1.4)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(3)])
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        for r in range(3):
            ens.replica(r).upload(*ic.lattice_of(case, 0 if r == 1 else 1))
        e.upload(*lat0)
        for h in (ens, e):
            h.set_thermal_substeps(3)
            h.set_thermal_scheme("implicit")
        ens.set_beam([ta, tb], [0, 1, 0])
        e.set_beam(tb)
        for (s0, n, _up, _ud, _unp, _q) in calls:
            res = ens.run(s0, n, 0.0, rng_mode=2, seeds=[5, case["seed"], 6], thermal_mode=2)
            rg = e.run_steps(s0, n, 0.0, None, None, None, rng_mode=2, seed=case["seed"], thermal_mode=2)
            assert (int(res["done"][1]), int(res["status"][1])) == (rg["done"], rg["status"]) == (n, 0)
            assert res["totals"][1][:n].tobytes() == rg["totals"].tobytes()
            a, b = ens.replica(1).download(defects=True), e.download(defects=True)
            for f in a:
                assert a[f].tobytes() == b[f].tobytes(), f
        assert e.beam_info() == ens.beam_info() and e.beam_info()["updates"] >= 2
        ens.replica(1).thermal_beam(1e-6, tb["u0"] + 1, use_latent=True, scrub_nan=True)
        e.thermal_beam(1e-6, tb["u0"] + 1, use_latent=True, scrub_nan=True)
        assert ens.replica(1).download()["T"].tobytes() == e.download()["T"].tobytes()
    finally:
        e.close()
        ens.close()
