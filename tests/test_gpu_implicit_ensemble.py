"""The implicit scheme in replica ensembles (cetkmc_ensemble_set_thermal_scheme + cetkmc_run_ensemble): every replica against
the comparator tests/implicit_ref.py after every call, L = 30 (R = 3, reference streams, n = 1) and L = 33 (R = 70,
counter-based uniforms, n = 3), two laser plane sets, a replica that terminates in the first call and is frozen in the second,
an empty replica; and a replica's bytes against a single handle's.  (The same kernels: R replicas only add lines.)"""
import numpy as np
import pytest

import remelt_cases as rc
import implicit_cases as sc
from helpers import assert_ensemble_call_matches_oracle
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1
POWERS = sc.POWERS


@pytest.mark.parametrize("name,R", [("ens_L30_n1", 3), ("ens_L33_n3", 70)])
def test_every_replica_vs_comparator(oracle_mod, name, R):
    import cetkmc
    case, runs = sc.replica_runs(name, R)
    L, n_calls = case["L"], len(case["batches"])
    assert runs[0][0]["results"][0]["status"] == 1 and runs[0][0]["results"][0]["done"] == 0      # terminates, then frozen
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(R)])
    try:
        for r, (run, _) in enumerate(runs):
            ens.replica(r).upload(*run["lat0"])
        ens.set_thermal_substeps(case["n_sub"])
        ens.set_thermal_scheme("implicit")
        q_set = np.array([s for _, s in runs], np.int32)
        updates = 0
        for c in range(n_calls):
            calls = [run["calls"][c] for run, _ in runs]
            s0, n = calls[0][0], calls[0][1]
            q = np.stack([rc.calls_of(case, p)[c][5] for p in POWERS])
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
            for r, ro in enumerate(ros):
                if ro is not None and "q_used" in ro:
                    assert int(res["q_used"][r]) == ro["q_used"], (r, res["q_used"][r], ro["q_used"])
            updates += updates_in(s0, n)
            assert ens.implicit_info() == dict(updates=updates, steps=updates * case["n_sub"], launches=3 * updates * case["n_sub"], coeff_uploads=1)
            assert ens.substep_info() == dict(updates=0, substeps=0, launches=0, blocked_launches=0)
        assert updates >= 2
    finally:
        ens.close()


def test_replica_bytes_equal_a_single_handle(oracle_mod):
    """the same lattice, calls and seed on a single handle and as replica 1 of three, n = 3"""
    import cetkmc
    case = sc.ENSEMBLE["ens_L33_n3"]
    L = case["L"]
    lat0 = sc.lattice_of(case)
    calls = rc.calls_of(case)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(3)])
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        for r in range(3):
            ens.replica(r).upload(*sc.lattice_of(case, 0 if r == 1 else 1))
        e.upload(*lat0)
        ens.set_thermal_substeps(3)
        e.set_thermal_substeps(3)
        ens.set_thermal_scheme("implicit")
        e.set_thermal_scheme("implicit")
        for (s0, n, _up, _ud, _unp, q) in calls:
            res = ens.run(s0, n, 0.0, rng_mode=2, seeds=[5, case["seed"], 6], thermal_mode=2, q_planes=q[None], q_set=[0, 0, 0])
            rg = e.run_steps(s0, n, 0.0, None, None, None, rng_mode=2, seed=case["seed"], thermal_mode=2, q_planes=q)
            assert (int(res["done"][1]), int(res["status"][1])) == (rg["done"], rg["status"]) == (n, 0)
            assert res["totals"][1][:n].tobytes() == rg["totals"].tobytes()
            a, b = ens.replica(1).download(defects=True), e.download(defects=True)
            for f in a:
                assert a[f].tobytes() == b[f].tobytes(), f
        assert e.implicit_info() == ens.implicit_info() and e.implicit_info()["updates"] >= 2
    finally:
        e.close()
        ens.close()
