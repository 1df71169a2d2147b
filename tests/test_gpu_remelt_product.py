"""Remelting in the product layer: run_kmc(remelt=) repeatable with its columns and last_run_info, a resume bit-identical,
remelt=False = the call without the keyword file by file, solid_metrics beside it, run_kmc_ensemble with the shared ``remelt``
key against sequential run_kmc calls, the refused combinations and the two driver flags."""
import os
import runpy
import sys

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

LASER = dict(power=150.0, start=2.0, speed=0.5)
KW = dict(L=24, n_steps=130, impurity_c=0.1, defect_fraction=3e-3, metrics_every=50)


def _files(prefix):
    d = os.path.join("outputs", prefix)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}


def test_run_kmc_laser_remelt_repeatable_with_columns(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    a = kmc_simulation.run_kmc(laser=LASER, remelt=True, output_prefix="a_0", **KW)
    info = dict(kmc_simulation.last_run_info)
    b = kmc_simulation.run_kmc(laser=LASER, remelt=True, output_prefix="b_0", **KW)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert open("outputs/a_0/metrics.csv", "rb").read() == open("outputs/b_0/metrics.csv", "rb").read()
    m = pd.read_csv("outputs/a_0/metrics.csv")
    assert list(m.columns[-2:]) == ["RemeltPasses", "RemeltedVoxels"] and "Remelted" not in m.columns
    # rows after steps 0, 50, 100, 129: the updates of steps 0; 0..40; 0..100; 0..120
    assert list(m["RemeltPasses"]) == [1, 3, 6, 7]
    assert (np.diff(m["RemeltedVoxels"]) >= 0).all() and m["RemeltedVoxels"].iloc[-1] > 0
    assert info["remelted"] == m["RemeltedVoxels"].iloc[-1] == kmc_simulation.last_run_info["remelted"]
    # the beam melts what it passes over: the run differs from the one without remelting, whose files have no such columns
    plain = kmc_simulation.run_kmc(laser=LASER, output_prefix="plain_0", **KW)
    assert not np.array_equal(plain[0], a[0]) and "remelted" not in kmc_simulation.last_run_info
    assert "RemeltPasses" not in pd.read_csv("outputs/plain_0/metrics.csv").columns


def test_remelt_false_is_the_call_without_the_keyword(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(KW, laser=LASER, front_metrics=True, solid_metrics=True)
    a = kmc_simulation.run_kmc(output_prefix="x_0", **kw)
    files_a = _files("x_0")
    os.rename("outputs/x_0", "outputs/kept_0")
    b = kmc_simulation.run_kmc(remelt=False, output_prefix="x_0", **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert _files("x_0") == files_a and len(files_a) >= 3


def test_resume_is_bit_identical(tmp_path, monkeypatch):
    """no laser (a checkpoint does not carry prev_state), a threshold inside the initial field's range"""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(KW, remelt=3300.0)
    whole = kmc_simulation.run_kmc(output_prefix="whole_0", **kw)
    total = kmc_simulation.last_run_info["remelted"]
    assert total > 0
    # the first part ends on a metrics step (50), so that it writes no row the whole run does not have
    kmc_simulation.run_kmc(output_prefix="part_0", checkpoint_every=51, **dict(kw, n_steps=51))
    rest = kmc_simulation.run_kmc(output_prefix="part_0", resume_from="outputs/part_0/checkpoint.npz", **kw)
    for x, y in zip(whole, rest):
        assert np.array_equal(x, y)
    assert open("outputs/whole_0/metrics.csv", "rb").read() == open("outputs/part_0/metrics.csv", "rb").read()
    assert kmc_simulation.last_run_info["remelted"] == total
    with pytest.raises(ValueError, match="remelt"):          # the checkpoint carries the setting
        kmc_simulation.run_kmc(output_prefix="part_0", resume_from="outputs/part_0/checkpoint.npz", **dict(kw, remelt=3400.0))
    with pytest.raises(ValueError, match="remelt"):
        kmc_simulation.run_kmc(output_prefix="part_0", resume_from="outputs/part_0/checkpoint.npz", **dict(kw, remelt=False))


def test_solid_metrics_beside_remelting(tmp_path, monkeypatch):
    """the solidification map sees a melt as occupied -> empty at its next update: ``Remelted`` >= the melted voxels that held
    a record.  With metrics_every = 20 run_kmc executes every temperature-update step g as a call of its own, right behind
    the map update at g; the test wraps Engine.run_steps and, around each such call, reads the state and the map's stamps:
    the voxels that were occupied before and are empty after are the melted ones (and the source of the step's own event, if
    that was a diffusion, which is taken out), those of them with stamp >= 0 held a record.  A melt is seen by the map
    update 20 steps later, so the melts of the last update the run reaches are left out of the bound."""
    import cetkmc
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    n_steps = 130
    seen = {}                              # update step -> melted voxels that held a record (summed over retried calls)
    inner = cetkmc.Engine.run_steps

    def run_steps(self, step0, n, *a, **kw):
        if not (n == 1 and step0 % 20 == 0):
            return inner(self, step0, n, *a, **kw)
        before, stamp = self.download(theta=False, phi=False, T=False)["state"], self.solid_read()["stamp"]
        r = inner(self, step0, n, *a, **kw)
        gone = (before != 0) & (self.download(theta=False, phi=False, T=False)["state"] == 0)
        if r["done"] == 1 and r["events"]["type"][0] == 1:
            gone[tuple(r["events"]["pos"][0])] = False
        seen[step0] = seen.get(step0, 0) + int((gone & (stamp >= 0)).sum())
        return r

    monkeypatch.setattr(cetkmc.Engine, "run_steps", run_steps)
    kmc_simulation.run_kmc(laser=LASER, remelt=True, solid_metrics=True, output_prefix="s_0", **dict(KW, n_steps=n_steps, metrics_every=20))
    m = pd.read_csv("outputs/s_0/metrics.csv")
    assert list(m.columns[-2:]) == ["RemeltPasses", "RemeltedVoxels"] and "Remelted" in m.columns
    assert sorted(seen) == list(range(0, n_steps, 20))
    last_map_update = (n_steps // 20) * 20
    with_record = sum(c for g, c in seen.items() if g + 20 <= last_map_update)
    print(f"melted voxels that held a record, per update step: {seen}; seen by the map: {with_record}; "
          f"Remelted {int(m['Remelted'].iloc[-1])}, RemeltedVoxels {int(m['RemeltedVoxels'].iloc[-1])}")
    assert with_record >= 1                                    # the input melts deposit, not only substrate
    assert m["Remelted"].iloc[-1] >= with_record


def test_ensemble_vs_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, n = 16, 130
    cfgs = [dict(impurity_c=0.1, seed=42 + s, defect_fraction=3e-3, output_prefix=f"e{s}_{s}", remelt=True,
                 laser=dict(power=100.0 + 30.0 * s, start=4.0, speed=0.5)) for s in range(3)]
    outs = kmc_simulation.run_kmc_ensemble(cfgs, L, n, metrics_every=50)
    infos = list(kmc_simulation.last_ensemble_info)
    for r, cfg in enumerate(cfgs):
        ref = kmc_simulation.run_kmc(L=L, n_steps=n, metrics_every=50, **dict(cfg, output_prefix="seq_" + cfg["output_prefix"]))
        for a, b in zip(outs[r], ref):
            assert np.array_equal(a, b), r
        a, b = (os.path.join("outputs", p + cfg["output_prefix"], "metrics.csv") for p in ("", "seq_"))
        assert open(a, "rb").read() == open(b, "rb").read(), r
        assert infos[r]["remelted"] == kmc_simulation.last_run_info["remelted"]
    assert sum(i["remelted"] for i in infos) > 0


def test_refused_combinations(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    for kw in (dict(mode="B", box=8), dict(origin_metrics=True), dict(thermal_updates=False), dict(remelt=float("nan")), dict(remelt="yes")):
        with pytest.raises(ValueError, match="remelt"):
            kmc_simulation.run_kmc(**{**dict(L=8, n_steps=5, remelt=True), **kw})
    ens = kmc_simulation.run_kmc_ensemble
    with pytest.raises(ValueError, match="remelt"):
        ens([dict(output_prefix="a", remelt=True), dict(output_prefix="b")], 8, 5)
    with pytest.raises(ValueError, match="remelt"):
        ens([dict(output_prefix="a", remelt=True)], 8, 5, rng="counter")
    with pytest.raises(ValueError, match="remelt"):
        ens([dict(output_prefix="a", remelt=True)], 8, 5, origin_metrics=True)
    assert not os.path.exists("outputs")                                 # refused before anything ran


def test_driver_flags(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["gv_sweep.py", "--L", "12", "--steps", "60", "--temps", "2800", "--nu-dep", "2e13", "--carbon", "0.1",
                                      "--laser-power", "150", "--scan-speed", "0.5", "--remelt"])
    runpy.run_module("gv_sweep", run_name="__main__")
    m = pd.read_csv("outputs/gv_sweep/T2800_V2e+13_P150_S0.5_c_10/metrics.csv")
    assert list(m.columns[-2:]) == ["RemeltPasses", "RemeltedVoxels"] and m["RemeltPasses"].iloc[-1] == 3
    monkeypatch.setattr(sys, "argv", ["main.py", "--L", "12", "--steps", "45", "--levels", "0.1", "--remelt", "3300"])
    runpy.run_module("main", run_name="__main__")
    m = pd.read_csv("outputs/impurity_c_10/metrics.csv")
    assert list(m.columns[-2:]) == ["RemeltPasses", "RemeltedVoxels"] and m["RemeltPasses"].iloc[-1] == 3
    capsys.readouterr()
