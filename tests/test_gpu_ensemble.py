"""Replica ensembles (cetkmc.Ensemble / kmc_simulation.run_kmc_ensemble): every replica reproduces the single run it
stands for -- reference fixtures, sequential run_kmc calls in both RNG settings -- whatever its companions do."""
import io
import os
import random

import numpy as np
import pandas as pd
import pytest

from helpers import load

pytestmark = pytest.mark.gpu


def _kw(z, name):
    kw = dict(temp=float(z["temp"]), defect_fraction=float(z["defect_fraction"]), n_seeds=int(z["n_seeds"]),
              impurity_c=float(z["impurity_c"]), output_prefix=name)
    if float(z["temp"]) == int(z["temp"]):
        kw["temp"] = int(z["temp"])
    return kw


def _same_csv(a, b):
    ga, gb = pd.read_csv(a), pd.read_csv(b)
    assert list(ga.columns) == list(gb.columns) and len(ga) == len(gb)
    for col in ga.columns:
        assert ga[col].tolist() == gb[col].tolist() or np.array_equal(ga[col].values, gb[col].values, equal_nan=True), col


def _check_fixture(z, name, out, info):
    state, atom_type, total_time, theta, phi = out
    assert np.array_equal(state, z["final_state"]) and np.array_equal(atom_type, state)
    assert np.array_equal(theta, z["final_theta"]) and np.array_equal(phi, z["final_phi"])
    assert total_time == float(z["total_time"])
    random.setstate(info["random_state"])
    np.random.set_state(info["np_state"])
    assert np.array_equal(np.array([random.random() for _ in range(4)]), z["py_next"])
    assert np.array_equal(np.random.random(4), z["np_next"])
    got = pd.read_csv(os.path.join("outputs", name, "metrics.csv"))
    want = pd.read_csv(io.StringIO(str(z["metrics_csv"])))
    assert list(got.columns) == list(want.columns) and len(got) == len(want)
    for col in want.columns:
        if want[col].dtype.kind == "f":
            assert np.allclose(got[col].values, want[col].values, rtol=1e-12, atol=0), col
        else:
            assert got[col].tolist() == want[col].tolist(), col


@pytest.mark.parametrize("name", ["traj_L9_n2500", "traj_L14_n2500", "traj_L30_n3"])
def test_fixture_replica0(name, tmp_path, monkeypatch):
    """Replica 0 of a 4-replica ensemble reproduces the reference fixture; its companions differ in seed, impurity_c,
    defect_fraction and temp."""
    import kmc_simulation
    z = load(name)
    monkeypatch.chdir(tmp_path)
    kw = _kw(z, name)
    comp = [dict(kw, output_prefix=f"c{i}_{i}", seed=7 + i, impurity_c=0.05 * (i + 1), defect_fraction=0.01 * i,
                 temp=2800 + 100 * i) for i in range(3)]
    outs = kmc_simulation.run_kmc_ensemble([kw] + comp, int(z["L"]), int(z["n_steps"]))
    _check_fixture(z, name, outs[0], kmc_simulation.last_ensemble_info[0])


def test_frozen_replica_unfreezes_on_new_lattice():
    """A terminated replica stays frozen (status 1, no steps) until a new lattice is uploaded into it."""
    import cetkmc
    L = 4
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(), cetkmc.default_params()])
    try:
        full = np.ones((L,) * 3, np.int64)                  # nothing can happen on a full lattice: terminates at once
        empty = np.zeros((L,) * 3, np.int64)
        T = np.full((L,) * 3, 2800.0)
        z = np.zeros((L,) * 3)
        ens.replica(0).upload(full, z, z, T, empty)
        ens.replica(1).upload(empty, z, z, T, empty)
        r1 = ens.run(0, 5, np.zeros(2), rng_mode=2, seeds=[1, 2], thermal_mode=0)
        assert r1["status"][0] == 1 and r1["done"][0] == 0 and r1["done"][1] == 5
        r2 = ens.run(5, 5, np.zeros(2), rng_mode=2, seeds=[1, 2], thermal_mode=0)
        assert r2["status"][0] == 1 and r2["done"][0] == 0
        ens.replica(0).upload(empty, z, z, T, empty)
        r3 = ens.run(10, 5, np.zeros(2), rng_mode=2, seeds=[1, 2], thermal_mode=0)
        assert r3["status"][0] == 0 and r3["done"][0] == 5
    finally:
        ens.close()


def test_termination_isolated(tmp_path, monkeypatch):
    """Replica 0 terminates at the fixture's step with its arrays; each companion (at 4^3 they fill up too, each at its own
    step) equals its own sequential run_kmc -- one of them steps on after replica 0 has frozen."""
    import kmc_simulation
    name = "traj_L4_n200_T3688_terminates"
    z = load(name)
    monkeypatch.chdir(tmp_path)
    kw = _kw(z, name)
    comp = [dict(kw, output_prefix=f"c{i}_{i}", temp=2800, seed=11 + i) for i in range(3)]
    L, n = int(z["L"]), int(z["n_steps"])
    outs = kmc_simulation.run_kmc_ensemble([kw] + comp, L, n)
    _check_fixture(z, name, outs[0], kmc_simulation.last_ensemble_info[0])
    info = list(kmc_simulation.last_ensemble_info)
    assert max(x["executed_events"] for x in info[1:]) > info[0]["executed_events"]
    for i, c in enumerate(comp):
        ref = kmc_simulation.run_kmc(L=L, n_steps=n, **dict(c, output_prefix=f"s{i}_{i}"))
        assert kmc_simulation.last_run_info["executed_events"] == info[1 + i]["executed_events"]
        for a, b in zip(outs[1 + i], ref):
            assert np.array_equal(a, b)
        _same_csv(os.path.join("outputs", c["output_prefix"], "metrics.csv"), os.path.join("outputs", f"s{i}_{i}", "metrics.csv"))


def _vs_sequential(configs, L, n, rng, tmp_path, monkeypatch, **seq_kw):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    random.seed(123)
    np.random.seed(321)
    py0, np0 = random.getstate(), np.random.get_state()
    outs = kmc_simulation.run_kmc_ensemble(configs, L, n, rng=rng)
    assert random.getstate() == py0                       # the caller's generators are left alone
    assert np.array_equal(np.random.get_state()[1], np0[1]) and np.random.get_state()[2] == np0[2]
    infos = list(kmc_simulation.last_ensemble_info)
    for r, c in enumerate(configs):
        ref = kmc_simulation.run_kmc(L=L, n_steps=n, **dict(c, output_prefix="seq_" + c["output_prefix"]), **seq_kw)
        for a, b in zip(outs[r], ref):
            assert np.array_equal(a, b), (r, c)
        _same_csv(os.path.join("outputs", c["output_prefix"], "metrics.csv"),
                  os.path.join("outputs", "seq_" + c["output_prefix"], "metrics.csv"))
        if rng == "reference":
            assert random.getstate() == infos[r]["random_state"]
            assert np.array_equal(np.random.get_state()[1], infos[r]["np_state"][1])
            assert np.random.get_state()[2] == infos[r]["np_state"][2]
    return outs


def test_reference_mode_vs_sequential_L30(tmp_path, monkeypatch):
    """3 carbon levels x 2 seeds at L = 30, 1100 steps: defect refreshes and 55 temperature updates crossed."""
    cfgs = [dict(impurity_c=c, seed=42 + s, defect_fraction=3e-3, output_prefix=f"ic_{c}_{s}")
            for c in (0.0, 0.1, 0.3) for s in range(2)]
    _vs_sequential(cfgs, 30, 1100, "reference", tmp_path, monkeypatch)


@pytest.mark.parametrize("L", [16, 30])
def test_counter_mode_vs_mode_b_single_domain(L, tmp_path, monkeypatch):
    cfgs = [dict(impurity_c=0.05 * (r % 4), seed=100 + r, defect_fraction=2e-3 * (r % 2), temp=2900 + 50 * (r % 3),
                 output_prefix=f"cn_{r}") for r in range(8)]
    _vs_sequential(cfgs, L, 450, "counter", tmp_path, monkeypatch, mode="B", box=L, thermal_cadence="supersteps")


def test_replica_independent_of_R_and_index(tmp_path, monkeypatch):
    """The same config at index 0 of R = 1 and at index 37 of R = 64 (companions shuffled) gives the same run."""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    me = dict(impurity_c=0.1, seed=5, defect_fraction=1e-3, output_prefix="me_x")
    rng = np.random.RandomState(9)
    others = [dict(impurity_c=float(rng.choice([0.0, 0.2, 0.3])), seed=int(rng.randint(1000)), temp=int(rng.choice([2700, 3000])),
                   output_prefix=f"o_{i}") for i in range(63)]
    for mode in ("reference", "counter"):
        a = kmc_simulation.run_kmc_ensemble([me], 12, 300, rng=mode)[0]
        cfgs = list(others)
        rng.shuffle(cfgs)
        cfgs.insert(37, dict(me, output_prefix="me_y"))
        b = kmc_simulation.run_kmc_ensemble(cfgs, 12, 300, rng=mode)[37]
        for u, v in zip(a, b):
            assert np.array_equal(u, v), mode
        _same_csv(os.path.join("outputs", "me_x", "metrics.csv"), os.path.join("outputs", "me_y", "metrics.csv"))


def test_batched_analysis_equals_engine():
    """Ensemble.analyze / set_defects_sparse (launches independent of R) equal the single-Engine clusters (labels, sizes,
    bounding boxes, first voxels), species counts, nucleation counts, carbon gather and defect scatter."""
    import cetkmc
    import lattice_init
    L, R = 14, 5
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1 * r) for r in range(R)])
    try:
        for r in range(R):
            np.random.seed(r)
            st, th, ph, T, _ = lattice_init.initialize_lattice(lattice_size=L, n_seeds=3, impurity_c=0.1 * r)
            ens.replica(r).upload(st, th, ph, T, np.zeros_like(st))
        ens.run(0, 60, np.full(R, 2e-3), rng_mode=2, seeds=np.arange(R), thermal_mode=1)
        an = ens.analyze(0.5, species=3, labels=True)
        rng = np.random.RandomState(1)
        lists = [None if r == 2 else np.sort(rng.choice(L ** 3, size=7 * r, replace=False)) for r in range(R)]
        ens.set_defects_sparse(lists)
        for r in range(R):
            rep = ens.replica(r)
            f = rep.download(defects=True)
            e = cetkmc.Engine(L, impurity_c=0.1 * r)
            e.upload(f["state"], f["theta"], f["phi"], f["T"], np.zeros_like(f["state"]))
            b = e.clusters(0.5, labels=True)
            for k in ("first", "size", "bbox", "labels"):
                assert np.array_equal(an[r]["clusters"][k], b[k]), (r, k)
            assert np.array_equal(an[r]["counts"], e.species_counts())
            assert an[r]["nucleation_count"] == rep.nucleation_count()
            for u, v in zip(an[r]["gather"], e.gather_species(3)):
                assert np.array_equal(u, v)
            if lists[r] is not None:
                e.set_defects_sparse(lists[r])
                assert np.array_equal(f["defects"], e.download(state=False, theta=False, phi=False, T=False, defects=True)["defects"])
            else:
                assert not f["defects"].any()          # left alone: nothing was ever set
            e.close()
    finally:
        ens.close()


def test_drivers_ensemble_writes_sequential_files(tmp_path, monkeypatch):
    """main.py --ensemble and gv_sweep.py --ensemble --seeds 2 (rng reference) write the files of the sequential runs."""
    import gv_sweep
    import main as driver
    seq, ens = tmp_path / "seq", tmp_path / "ens"
    for d, flag in ((seq, False), (ens, True)):
        d.mkdir()
        monkeypatch.chdir(d)
        driver.main(12, 450, (0.0, 0.2), ensemble=flag)
        gv_sweep.gv_sweep(12, 250, (2800.0, 3100.0), (2e12, 2e13), 0.1, seeds=2, ensemble=flag)
    files = sorted(p.relative_to(seq) for p in seq.rglob("*") if p.is_file())
    assert any(p.name == "gv_map.csv" for p in files) and any(p.name == "metrics.csv" for p in files)
    assert "seed" in pd.read_csv(seq / "outputs" / "gv_sweep" / "gv_map.csv").columns
    for p in files:
        assert (ens / p).read_bytes() == (seq / p).read_bytes(), p


def test_errors_not_faults():
    import cetkmc
    from cetkmc import _lib
    import ctypes as C
    with pytest.raises(RuntimeError, match="L <= 128"):
        cetkmc.Ensemble(129, [cetkmc.default_params()])
    with pytest.raises(RuntimeError, match="R >= 1"):
        cetkmc.Ensemble(8, [])
    with pytest.raises(RuntimeError, match="too many replicas"):           # grid limit (z = replica x plane groups)
        cetkmc.Ensemble(128, [cetkmc.default_params()] * 2100)
    p = cetkmc.default_params()
    q = cetkmc.default_params()
    q.kT = p.kT * 1.01
    with pytest.raises(RuntimeError, match="impurity_c and nu_dep only"):
        cetkmc.Ensemble(8, [p, q])
    ens = cetkmc.Ensemble(8, [cetkmc.default_params(), cetkmc.default_params(0.2)])
    try:
        with pytest.raises(RuntimeError, match="thermal_mode"):
            ens.run(0, 5, np.zeros(2), rng_mode=2, seeds=[1, 2], thermal_mode=2)
        with pytest.raises(RuntimeError, match="rng_mode"):
            ens.run(0, 5, np.zeros(2), rng_mode=1, seeds=[1, 2])
        with pytest.raises(RuntimeError, match="np_stride"):
            ens.run(0, 5, np.zeros(2), np.zeros((2, 5)), None, np.zeros((2, 10)), rng_mode=0)
        lib = _lib.load()
        assert lib.cetkmc_destroy(ens.replica(1).h) != 0          # a replica belongs to its ensemble
        with pytest.raises(RuntimeError, match="cetkmc_run_ensemble"):      # replicas are stepped by the ensemble only
            ens.replica(0).run_steps(0, 2, 0.0, None, None, None, rng_mode=2)
        e = cetkmc.Engine(8)
        out = C.c_void_p()
        assert lib.cetkmc_ensemble_replica(e.h, 0, C.byref(out)) != 0     # single-lattice handles refuse it
        e.close()
    finally:
        ens.close()
