"""The laser thermal mode in the product layer: run_kmc(laser=) against a loop composed on the host from the oracle,
run_kmc_ensemble with laser configs against sequential run_kmc(laser=) calls, the refused combinations, and the laser axes
of gv_sweep.py."""
import os
import random
import runpy
import sys

import numpy as np
import pandas as pd
import pytest

from test_gpu_ensemble import _same_csv
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

LASER = dict(power=150.0, start=2.0, speed=0.5)


def _oracle_run_kmc(o, L, n_steps, laser, defect_fraction, impurity_c, metrics_every, seed=42, temp=2800, n_seeds=5):
    """run_kmc(laser=) re-enacted on the host: the reference's prefix and generators (kmc_simulation.py:222-227), then per
    stretch between two metrics rows one oracle.Lattice.run_steps(thermal_mode=2) call fed from the same generators in the
    order the reference draws from them, source planes from oracle.laser_source_plane, the defect-mask refresh of
    kmc_simulation.py:335-338 on the multiples of metrics_every.  Returns state, theta, phi, total_time."""
    import defects as host_defects
    import lattice_init as host_init
    np.random.seed(seed)
    random.seed(seed)
    state, theta, phi, T, atom = host_init.initialize_lattice(lattice_size=L, n_seeds=n_seeds, T_sub=temp, impurity_c=impurity_c)
    mask, _ = host_defects.introduce_defects(state, atom, T, apply_to_state=False)
    lat = o.Lattice(state, theta, phi, T, mask, impurity_c=impurity_c)
    per = 3 if defect_fraction > 0.0 else 2
    total_time, next_step = 0.0, 0
    while next_step < n_steps:
        stop = next_step if next_step % metrics_every == 0 else min((next_step // metrics_every + 1) * metrics_every, n_steps - 1)
        stop = min(stop, n_steps - 1)
        n = stop - next_step + 1
        draws = np.array([random.random() for _ in range(per * n)]).reshape(n, per)
        np_state = np.random.get_state()
        u_np = np.random.random(n * (L * L + 2))
        us = [g // 20 for g in range(next_step, next_step + n) if g % 20 == 0]
        q = np.array([o.laser_source_plane(L, (laser["start"] + laser["speed"] * u,) * 2, laser["power"]) for u in us]).reshape(len(us), L, L)
        ro = lat.run_steps(next_step, n, defect_fraction, draws[:, 0], draws[:, 1] if per == 3 else None, u_np, rng_mode=0,
                           thermal_mode=2, q_planes=q if len(us) else None)
        assert ro["status"] == 0 and ro["done"] == n and ro["q_used"] == len(us), ro      # (a run that stops early is not this test)
        np.random.set_state(np_state)
        if ro["np_used"]:
            np.random.random(ro["np_used"])
        for s in range(n):
            total_time += max(-np.log(max(1e-12, draws[s, per - 1])) / ro["totals"][s], 1e-12)
        if stop % metrics_every == 0:
            s_now = lat.state.astype(np.int64)
            mask, _ = host_defects.introduce_defects(s_now, s_now, lat.T, apply_to_state=False)
            lat.defects = np.ascontiguousarray(mask, dtype=np.int8)
        next_step = stop + 1
    return lat, total_time


def test_run_kmc_laser_vs_oracle(oracle_mod, tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, n, df, c, me = 12, 130, 0.05, 0.2, 50
    state, atom_type, total_time, theta, phi = kmc_simulation.run_kmc(L=L, n_steps=n, defect_fraction=df, impurity_c=c, output_prefix="laser_0",
                                                                      laser=LASER, metrics_every=me)
    py_end, np_end = [random.random() for _ in range(4)], np.random.random(4)
    rows = pd.read_csv("outputs/laser_0/metrics.csv")
    assert rows["Step"].tolist() == [0, 50, 100, 129]
    lat, want_time = _oracle_run_kmc(oracle_mod, L, n, LASER, df, c, me)
    assert np.array_equal(state, lat.state) and np.array_equal(atom_type, state)
    assert np.array_equal(theta.view(np.int64), lat.theta.view(np.int64)) and np.array_equal(phi.view(np.int64), lat.phi.view(np.int64))
    assert abs(total_time - want_time) <= RATE_RTOL * want_time, (total_time, want_time)      # a sum of dt = f(total), totals to RATE_RTOL
    assert py_end == [random.random() for _ in range(4)]
    assert np.array_equal(np_end, np.random.random(4))
    # the laser did act: the same run without it ends elsewhere
    plain = kmc_simulation.run_kmc(L=L, n_steps=n, defect_fraction=df, impurity_c=c, output_prefix="plain_0", metrics_every=me)
    assert not np.array_equal(plain[0], state)


def test_ensemble_vs_sequential_reference(tmp_path, monkeypatch):
    """3 (power, speed) points x 2 seeds at L = 16, 450 steps: arrays, metrics.csv bytes, generators."""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, n = 16, 450
    points = [(120.0, 0.5), (220.0, 0.5), (220.0, -0.25)]
    cfgs = [dict(impurity_c=0.1, seed=42 + s, defect_fraction=3e-3, output_prefix=f"p{i}_{s}", laser=dict(power=p, start=4.0, speed=v))
            for i, (p, v) in enumerate(points) for s in range(2)]
    random.seed(123)
    np.random.seed(321)
    py0, np0 = random.getstate(), np.random.get_state()
    outs = kmc_simulation.run_kmc_ensemble(cfgs, L, n)
    assert random.getstate() == py0
    assert np.array_equal(np.random.get_state()[1], np0[1]) and np.random.get_state()[2] == np0[2]
    infos = list(kmc_simulation.last_ensemble_info)
    for r, cfg in enumerate(cfgs):
        ref = kmc_simulation.run_kmc(L=L, n_steps=n, **dict(cfg, output_prefix="seq_" + cfg["output_prefix"]))
        for a, b in zip(outs[r], ref):
            assert np.array_equal(a, b), (r, cfg)
        a, b = (os.path.join("outputs", p + cfg["output_prefix"], "metrics.csv") for p in ("", "seq_"))
        assert open(a, "rb").read() == open(b, "rb").read(), r
        assert random.getstate() == infos[r]["random_state"]
        assert np.array_equal(np.random.get_state()[1], infos[r]["np_state"][1]) and np.random.get_state()[2] == infos[r]["np_state"][2]
    # the points differ, the seeds of a point differ
    assert not np.array_equal(outs[0][0], outs[2][0]) and not np.array_equal(outs[0][0], outs[1][0])


def test_counter_mode_same_config_at_two_indices(tmp_path, monkeypatch):
    """rng="counter": the same config as the only replica and as replica 5 of 9 -- same arrays, same CSV."""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, n = 12, 130
    mine = dict(impurity_c=0.2, seed=7, defect_fraction=0.01, output_prefix="one_0", laser=LASER)
    a = kmc_simulation.run_kmc_ensemble([mine], L, n, rng="counter", metrics_every=50)
    others = [dict(impurity_c=0.05 * i, seed=100 + i, output_prefix=f"o{i}_{i}", laser=dict(LASER, power=40.0 * (i + 1), speed=0.1 * i))
              for i in range(9)]
    others[5] = dict(mine, output_prefix="nine_5")
    b = kmc_simulation.run_kmc_ensemble(others, L, n, rng="counter", metrics_every=50)
    for x, y in zip(a[0], b[5]):
        assert np.array_equal(x, y)
    _same_csv("outputs/one_0/metrics.csv", "outputs/nine_5/metrics.csv")
    assert open("outputs/one_0/metrics.csv", "rb").read() == open("outputs/nine_5/metrics.csv", "rb").read()
    assert not np.array_equal(b[4][0], b[5][0])


def test_refused_combinations(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    run = kmc_simulation.run_kmc
    for kw in (dict(mode="B", box=8), dict(checkpoint_every=10), dict(resume_from="nowhere.npz"), dict(thermal_updates=False)):
        with pytest.raises(ValueError, match="laser"):
            run(L=8, n_steps=5, laser=LASER, **kw)
    with pytest.raises(ValueError, match="laser"):
        run(L=8, n_steps=5, laser=dict(power=1.0))                       # start / speed missing
    ens = kmc_simulation.run_kmc_ensemble
    with pytest.raises(ValueError, match="every config has a laser or none"):
        ens([dict(output_prefix="a", laser=LASER), dict(output_prefix="b")], 8, 5)
    with pytest.raises(ValueError, match="thermal_updates"):
        ens([dict(output_prefix="a", laser=LASER)], 8, 5, thermal_updates=False)
    with pytest.raises(ValueError, match="latent"):
        ens([dict(output_prefix="a", laser=LASER), dict(output_prefix="b", laser=dict(LASER, latent=False))], 8, 5)
    assert not os.path.exists("outputs")                                 # refused before anything ran


def test_gv_sweep_laser_axes(tmp_path, monkeypatch, capsys):
    """gv_sweep.py --ensemble --laser-power a,b --scan-speed c,d: one row per point with power and speed columns; without
    the two flags the map has the columns and the run directories it had."""
    monkeypatch.chdir(tmp_path)
    base = ["gv_sweep.py", "--L", "12", "--steps", "60", "--temps", "2800", "--nu-dep", "2e13", "--carbon", "0.1", "--ensemble"]
    monkeypatch.setattr(sys, "argv", base + ["--laser-power", "100,200", "--scan-speed", "0.5,-0.5"])
    runpy.run_module("gv_sweep", run_name="__main__")
    m = pd.read_csv("outputs/gv_sweep/gv_map.csv")
    assert list(m.columns[:4]) == ["T_sub", "nu_dep", "power", "speed"] and len(m) == 4
    assert sorted(zip(m["power"], m["speed"])) == [(100.0, -0.5), (100.0, 0.5), (200.0, -0.5), (200.0, 0.5)]
    for p in (100, 200):
        for v in (0.5, -0.5):
            assert os.path.exists(f"outputs/gv_sweep/T2800_V2e+13_P{p}_S{v:g}_c_10/metrics.csv")
    monkeypatch.setattr(sys, "argv", base)
    runpy.run_module("gv_sweep", run_name="__main__")
    m0 = pd.read_csv("outputs/gv_sweep/gv_map.csv")
    assert list(m0.columns) == ["T_sub", "nu_dep", "G_K_per_m", "V_m_per_s", "G_over_V", "AspectRatio", "EquiaxedFraction", "GrainCount",
                                "NucleationCount", "CET_Class", "CET_Detected"] and len(m0) == 1
    assert os.path.exists("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv")
    capsys.readouterr()
