"""A thermal boundary in replica ensembles (cetkmc_ensemble_set_thermal_boundary + cetkmc_run_ensemble): every replica against
the comparator tests/boundary_ref.py after every call, L = 30 (R = 3, reference streams, n = 1) and L = 33 (R = 70, counter-based
uniforms, n = 3), two laser plane sets, a replica that terminates in the first call and is frozen in the second, an empty
replica; and a replica's bytes against a single handle's with the same boundary.  One boundary for all replicas: a substrate sink
whose temperature falls by 50 K per update and a convective top."""
import numpy as np
import pytest

import boundary_cases as bc
import implicit_cases as ic
import remelt_cases as rc
from helpers import assert_ensemble_call_matches_oracle
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


@pytest.mark.parametrize("name,R", [("ens_L30_n1_bc", 3), ("ens_L33_n3_bc", 70)])
def test_every_replica_vs_comparator(oracle_mod, name, R):
    import cetkmc
    case, runs = bc.replica_runs(name, R)
    L, n_calls, n_sub = case["L"], len(case["batches"]), case["n_sub"]
    assert runs[0][0]["results"][0]["status"] == 1 and runs[0][0]["results"][0]["done"] == 0      # terminates, then frozen
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(R)])
    try:
        for r, (run, _) in enumerate(runs):
            ens.replica(r).upload(*run["lat0"])
        ens.set_thermal_substeps(n_sub)
        ens.set_thermal_scheme("implicit")
        ens.set_thermal_boundary(bc.ENS_BC)
        q_set = np.array([s for _, s in runs], np.int32)
        updates = 0
        for c in range(n_calls):
            calls = [run["calls"][c] for run, _ in runs]
            s0, n = calls[0][0], calls[0][1]
            q = np.stack([rc.calls_of(case, p)[c][5] for p in bc.POWERS])
            kw = dict(thermal_mode=2, q_planes=q, q_set=q_set, use_latent=case["use_latent"])
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
            tot = dict(updates=updates, steps=updates * n_sub, launches=3 * updates * n_sub)
            assert ens.boundary_info() == dict(tot, coeff_uploads=1) and ens.implicit_info() == dict(tot, coeff_uploads=0)
        assert updates >= 2
        got = ens.thermal_boundary()
        assert all(np.array_equal(got[f], bc.ENS_BC[f]) for f in ("beta", "T_ext", "ramp"))
    finally:
        ens.close()


def test_replica_bytes_equal_a_single_handle(oracle_mod):
    """the same lattice, calls, seed and boundary on a single handle and as replica 1 of three, n = 3"""
    import cetkmc
    case = bc.ENSEMBLE["ens_L33_n3_bc"]
    L = case["L"]
    lat0 = ic.lattice_of(case)
    calls = rc.calls_of(case)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(3)])
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        for r in range(3):
            ens.replica(r).upload(*ic.lattice_of(case, 0 if r == 1 else 1))
        e.upload(*lat0)
        for h in (ens, e):
            h.set_thermal_substeps(3)
            h.set_thermal_scheme("implicit")
            h.set_thermal_boundary(bc.ENS_BC)
        for (s0, n, _up, _ud, _unp, q) in calls:
            res = ens.run(s0, n, 0.0, rng_mode=2, seeds=[5, case["seed"], 6], thermal_mode=2, q_planes=q[None], q_set=[0, 0, 0])
            rg = e.run_steps(s0, n, 0.0, None, None, None, rng_mode=2, seed=case["seed"], thermal_mode=2, q_planes=q)
            assert (int(res["done"][1]), int(res["status"][1])) == (rg["done"], rg["status"]) == (n, 0)
            assert res["totals"][1][:n].tobytes() == rg["totals"].tobytes()
            a, b = ens.replica(1).download(defects=True), e.download(defects=True)
            for f in a:
                assert a[f].tobytes() == b[f].tobytes(), f
        assert e.boundary_info() == ens.boundary_info() and e.boundary_info()["updates"] >= 2
        assert e.implicit_info() == ens.implicit_info()
    finally:
        e.close()
        ens.close()
