"""run_kmc_ensemble without a GPU: argument validation happens before any device call, and the per-replica host
prefix equals run_kmc's under the global generators (which the caller gets back untouched)."""
import random

import numpy as np
import pytest


def test_validation_before_device():
    import kmc_simulation as K
    with pytest.raises(ValueError, match="rng"):
        K.run_kmc_ensemble([{}], 8, 10, rng="fast")
    with pytest.raises(ValueError, match="L <= 128"):
        K.run_kmc_ensemble([{}], 129, 10)
    with pytest.raises(ValueError, match="L <= 128"):
        K.run_kmc_ensemble([{}], 0, 10)
    with pytest.raises(ValueError, match="n_steps"):
        K.run_kmc_ensemble([{}], 8, -1)
    with pytest.raises(ValueError, match="non-empty"):
        K.run_kmc_ensemble([], 8, 10)
    with pytest.raises(ValueError, match="unknown keys"):
        K.run_kmc_ensemble([{"mode": "B"}], 8, 10)
    with pytest.raises(ValueError, match="output_prefix"):
        K.run_kmc_ensemble([{"seed": 1}, {"seed": 2}], 8, 10)
    with pytest.raises(ValueError, match="metrics_every"):
        K.run_kmc_ensemble([{}], 8, 10, metrics_every=0)
    with pytest.raises(ValueError, match="defect_fraction"):
        K.run_kmc_ensemble([{"defect_fraction": -1.0}], 8, 10)


def test_replica_prefix_matches_run_kmc_prefix():
    """kmc_simulation.py:222-227 under the global generators vs the replica prefix, interleaved with other replicas."""
    import defects
    import kmc_simulation as K
    import lattice_init
    cfgs = K._ensemble_configs([dict(seed=3, impurity_c=0.2, temp=2900, n_seeds=4, output_prefix="a"),
                                dict(impurity_c=0.1, output_prefix="b")], 10, 50, "reference", 200)
    random.seed(999)
    np.random.seed(999)
    py0, np0 = random.getstate(), np.random.get_state()
    pre = [K._replica_prefix(c, 10) for c in cfgs]
    for c, p in zip(cfgs, pre):
        seed = 42 if c["seed"] is None else c["seed"]
        np.random.seed(seed)
        random.seed(seed)
        st, th, ph, T, atom = lattice_init.initialize_lattice(lattice_size=10, n_seeds=c["n_seeds"], T_sub=c["temp"],
                                                              impurity_c=c["impurity_c"])
        mask, _ = defects.introduce_defects(st, atom, T, apply_to_state=False)
        for k, v in (("state", st), ("theta", th), ("phi", ph), ("T", T), ("defects", mask)):
            assert np.array_equal(p[k], v), k
        assert p["py_state"] == random.getstate()
        assert np.array_equal(p["np_state"][1], np.random.get_state()[1]) and p["np_state"][2] == np.random.get_state()[2]
    # the swap helper hands a replica's states to the globals and takes the advanced ones back
    random.setstate(py0)
    np.random.set_state(np0)
    g = K._GlobalRNG(pre[0]["py_state"], pre[0]["np_state"])
    with g:
        x = (random.random(), np.random.random())
    random.setstate(pre[0]["py_state"])
    np.random.set_state(pre[0]["np_state"])
    assert x == (random.random(), np.random.random())
    assert g.py == random.getstate()


def test_caller_generators_restored_on_failure(monkeypatch):
    """A call that fails after the host prefix (here: the device handle cannot be created) leaves the caller's generator
    states as they were."""
    import cetkmc
    import kmc_simulation as K

    def no_device(*a, **k):
        raise RuntimeError("no device")
    monkeypatch.setattr(cetkmc, "Ensemble", no_device)
    random.seed(5)
    np.random.seed(5)
    py0, np0 = random.getstate(), np.random.get_state()
    with pytest.raises(Exception):
        K.run_kmc_ensemble([dict(output_prefix="x")], 6, 5)
    assert random.getstate() == py0 and np.array_equal(np.random.get_state()[1], np0[1])


def test_reference_budget_rejected():
    import kmc_simulation as K
    with pytest.raises(ValueError, match="split the ensemble"):
        K.run_kmc_ensemble([dict(output_prefix=f"p{i}") for i in range(2049)], 128, 10)


def test_driver_arguments_checked_before_device(monkeypatch):
    """main.py / gv_sweep.py: bad --ensemble / --rng / --seeds combinations fail before any run starts."""
    import gv_sweep
    import kmc_simulation
    import main as driver

    def no_run(*a, **k):
        raise AssertionError("a run started")
    for mod in (driver, gv_sweep, kmc_simulation):
        for name in ("run_kmc", "run_kmc_ensemble"):
            if hasattr(mod, name):
                monkeypatch.setattr(mod, name, no_run)
    with pytest.raises(ValueError, match="needs --ensemble"):
        driver.main(8, 10, (0.0,), rng="counter")
    with pytest.raises(ValueError, match="rng"):
        driver.main(8, 10, (0.0,), ensemble=True, rng="fast")
    with pytest.raises(ValueError, match="no run_kmc options"):
        driver.main(8, 10, (0.0,), ensemble=True, mode="B", box=8)
    with pytest.raises(ValueError, match="L <= 128"):
        driver.main(256, 10, (0.0,), ensemble=True)
    with pytest.raises(ValueError, match="same output directory"):
        driver.main(8, 10, (0.1, 0.101), ensemble=True)
    with pytest.raises(ValueError, match="seeds"):
        gv_sweep.gv_sweep(8, 10, (2800.0,), (2e12,), 0.1, seeds=0)
    with pytest.raises(ValueError, match="needs --ensemble"):
        gv_sweep.gv_sweep(8, 10, (2800.0,), (2e12,), 0.1, rng="counter")
    with pytest.raises(ValueError, match="no run_kmc options"):
        gv_sweep.gv_sweep(8, 10, (2800.0,), (2e12,), 0.1, ensemble=True, mode="B")
    with pytest.raises(ValueError, match="L <= 128"):
        gv_sweep.gv_sweep(200, 10, (2800.0,), (2e12,), 0.1, ensemble=True)
