"""Sub-stepped temperature updates in replica ensembles (cetkmc_ensemble_set_thermal_substeps + cetkmc_run_ensemble): every
replica against the comparator tests/substep_ref.py after every call, L = 30 (R = 3, reference streams, n = 3) and L = 33
(R = 70, counter-based uniforms, n = 17), two laser plane sets, a replica that terminates in the first call and is frozen in
the second, an empty replica; and a replica's bytes against a single handle's.  (Ensembles take the plain path: n launches of
k_thermal_march<EnsSel> per update.)"""
import numpy as np
import pytest

import remelt_cases as rc
import substep_cases as sc
from helpers import assert_ensemble_call_matches_oracle
from remelt_ref import updates_in
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1
POWERS = (60.0, 80.0)       # the two plane sets


def _full_cold(L):
    """no event anywhere (every voxel occupied): terminates in the call's first step"""
    rs = np.random.RandomState(77)
    state = rs.randint(1, 4, (L, L, L)).astype(np.int64)
    ang = rs.random_sample((L, L, L))
    return state, ang, 2 * ang, np.full((L, L, L), 3000.0), np.zeros_like(state)


def _empty(case):
    z = np.zeros((case["L"],) * 3)
    return z.astype(np.int64), z, z.copy(), rc.lattice_of(case)[3], z.astype(np.int64)


def _replica_runs(name, R):
    """per replica: (the comparator's run, plane set).  Replicas r >= 2 cycle through three (lattice, seed, plane set)
    combinations, so R = 70 costs three comparator runs; replica 0 terminates at once, replica 1 starts empty."""
    case = sc.ENSEMBLE[name]
    runs = [(sc.run_case(case, lat0=_full_cold(case["L"])), 0), (sc.run_case(case, power=POWERS[1], lat0=_empty(case)), 1)]
    for r in range(2, R):
        v = r % 3
        runs.append((sc.stepped(name, v, v, POWERS[v % 2]), v % 2))
    return case, runs


@pytest.mark.parametrize("name,R", [("ens_L30_n3", 3), ("ens_L33_n17", 70)])
def test_every_replica_vs_comparator(oracle_mod, name, R):
    import cetkmc
    case, runs = _replica_runs(name, R)
    L, n_calls = case["L"], len(case["batches"])
    assert runs[0][0]["results"][0]["status"] == 1 and runs[0][0]["results"][0]["done"] == 0      # terminates, then frozen
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(R)])
    try:
        for r, (run, _) in enumerate(runs):
            ens.replica(r).upload(*run["lat0"])
        ens.set_thermal_substeps(case["n_sub"])
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
            info = ens.substep_info()
            assert info == dict(updates=updates, substeps=updates * case["n_sub"], launches=updates * case["n_sub"], blocked_launches=0)
        assert updates >= 2
    finally:
        ens.close()


def test_replica_bytes_equal_a_single_handle(oracle_mod):
    """the same lattice, calls and seed on a single handle (cetkmc_set_thermal_substeps: the blocked kernel) and as replica 1
    of three (the plain path)"""
    import cetkmc
    case = sc.ENSEMBLE["ens_L33_n17"]
    L = case["L"]
    lat0 = rc.lattice_of(case)
    calls = rc.calls_of(case)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(3)])
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        for r in range(3):
            ens.replica(r).upload(*rc.lattice_of(case, 0 if r == 1 else 1))
        e.upload(*lat0)
        ens.set_thermal_substeps(17)
        e.set_thermal_substeps(17)
        e.set_option("substep_block", sc.S_DEFAULT)
        for (s0, n, _up, _ud, _unp, q) in calls:
            res = ens.run(s0, n, 0.0, rng_mode=2, seeds=[5, case["seed"], 6], thermal_mode=2, q_planes=q[None], q_set=[0, 0, 0])
            rg = e.run_steps(s0, n, 0.0, None, None, None, rng_mode=2, seed=case["seed"], thermal_mode=2, q_planes=q)
            assert (int(res["done"][1]), int(res["status"][1])) == (rg["done"], rg["status"]) == (n, 0)
            assert res["totals"][1][:n].tobytes() == rg["totals"].tobytes()
            a, b = ens.replica(1).download(defects=True), e.download(defects=True)
            for f in a:
                assert a[f].tobytes() == b[f].tobytes(), f
        assert e.substep_info()["blocked_launches"] > 0 and ens.substep_info()["blocked_launches"] == 0
    finally:
        e.close()
        ens.close()
