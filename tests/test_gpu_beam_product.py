"""Laser scan paths in the product layer: run_kmc(laser={..., "path": ...}, thermal_scheme="implicit")
repeatable, reported in last_run_info and composing with remelt, thermal_substeps, thermal_boundary and the diagnostics; a run cut
into two adjacent step ranges at the engine level reads the same rows; a laser dict without ``path`` stays on the plane route;
run_kmc_ensemble with one table per distinct laser dict against sequential run_kmc calls; the refused combinations and the
driver flags."""
import os
import runpy
import sys

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

RADIUS = 7.5e-6             # 1.5 voxels
PATH = dict(pattern="serpentine", speed=5.0, hatch=4.0, start=6.0, margin=4.0)
LASER = dict(power=0.6, path=PATH, beam_radius=RADIUS, depth=2)          # about 45 K per update at the peak
KW = dict(L=24, n_steps=130, impurity_c=0.1, defect_fraction=3e-3, metrics_every=50, thermal_scheme="implicit")


def _files(prefix):
    d = os.path.join("outputs", prefix)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}


def test_scan_is_repeatable_reported_and_composes(tmp_path, monkeypatch):
    import kmc_simulation
    import thermal_solver
    from constants import T_SUB
    monkeypatch.chdir(tmp_path)
    a = kmc_simulation.run_kmc(laser=LASER, output_prefix="a_0", **KW)
    info = kmc_simulation.last_run_info["beam"]
    assert info["path"] == PATH and info["depth"] == 2 and info["table_uploads"] == 1
    assert info["updates"] == 7 and info["launches"] == 21                 # steps 0, 20, .., 120
    b = kmc_simulation.run_kmc(laser=LASER, output_prefix="b_0", **KW)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert _files("a_0") == _files("b_0")
    sink = thermal_solver.thermal_boundary(bottom=("fixed", T_SUB))
    c = kmc_simulation.run_kmc(laser=dict(LASER, depth=4, penetration=1e-5, latent=False), remelt=True, thermal_substeps=3, thermal_boundary=sink,
                               front_metrics=True, solid_metrics=True, output_prefix="c_0", **KW)
    assert len(c) == len(a) and kmc_simulation.last_run_info["beam"]["steps"] == 21
    assert "RemeltedVoxels" in pd.read_csv("outputs/c_0/metrics.csv").columns
    # another power is another run
    d = kmc_simulation.run_kmc(laser=dict(LASER, power=1.2), output_prefix="d_0", **KW)
    assert _files("d_0")["metrics.csv"] != _files("a_0")["metrics.csv"] or not all(np.array_equal(x, y) for x, y in zip(a, d))


def test_without_a_path_the_plane_route_is_taken(tmp_path, monkeypatch):
    """the existing start / speed form: no table is built, nothing is reported, and the run is the repeatable run it was (the
    files of the plane route are pinned by tests/test_gpu_laser_product.py and its siblings, which stay as they are)"""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    plane = dict(power=150.0, start=2.0, speed=0.5)
    for scheme in ("explicit", "implicit"):
        a = kmc_simulation.run_kmc(laser=plane, output_prefix=f"a{scheme}_0", **dict(KW, thermal_scheme=scheme))
        assert "beam" not in kmc_simulation.last_run_info
        b = kmc_simulation.run_kmc(laser=plane, output_prefix=f"b{scheme}_0", **dict(KW, thermal_scheme=scheme))
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        assert _files(f"a{scheme}_0") == _files(f"b{scheme}_0")


def test_two_adjacent_step_ranges_read_the_same_rows():
    """steps [0, 140) under one table of seven rows, and cut at step 80 with the tables of ordinals [0, 4) and [4, 7)"""
    import cetkmc
    import implicit_cases as ic
    import kmc_simulation
    import thermal_solver
    L = 24
    lat0 = ic.lattice_of(ic.STEPPING["L24_laser_latent_rng0_full_n1"])
    path = thermal_solver.scan_path(L, **PATH)
    kw = dict(power=LASER["power"], beam_radius=RADIUS, depth=2)
    whole = kmc_simulation._beam_table_of(LASER, L, 140)
    assert whole["amp"].size == 7 and whole["amp"][-1] > 0
    out = []
    for tables in (((0, 140, whole),), ((0, 80, thermal_solver.beam_table(L, path, 0, 4, **kw)), (80, 60, thermal_solver.beam_table(L, path, 4, 3, **kw)))):
        e = cetkmc.Engine(L, impurity_c=0.1)
        try:
            e.upload(*lat0)
            e.set_thermal_scheme("implicit")
            tot = []
            for s0, n, t in tables:
                e.set_beam(t)
                r = e.run_steps(s0, n, 0.0, None, None, None, rng_mode=2, seed=11, thermal_mode=2)
                assert (r["done"], r["status"]) == (n, 0)
                tot.append(r["totals"])
            out.append((np.concatenate(tot), e.download(defects=True)))
        finally:
            e.close()
    assert out[0][0].tobytes() == out[1][0].tobytes()
    for f in out[0][1]:
        assert out[0][1][f].tobytes() == out[1][1][f].tobytes(), f


def test_ensemble_vs_sequential(tmp_path, monkeypatch):
    """three replicas, two distinct laser dicts (two tables, replicas 0 and 2 share one)"""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, n = 16, 130
    path = dict(pattern="raster", speed=4.0, hatch=3.0, margin=2.0)
    cfgs = [dict(impurity_c=0.1, seed=42 + s, defect_fraction=3e-3, output_prefix=f"e{s}_{s}",
                 laser=dict(power=0.5 + 0.3 * (s % 2), path=path, beam_radius=RADIUS, depth=3, penetration=1e-5)) for s in range(3)]
    outs = kmc_simulation.run_kmc_ensemble(cfgs, L, n, metrics_every=50, thermal_scheme="implicit")
    for r, cfg in enumerate(cfgs):
        ref = kmc_simulation.run_kmc(L=L, n_steps=n, metrics_every=50, thermal_scheme="implicit", **dict(cfg, output_prefix="seq_" + cfg["output_prefix"]))
        for a, b in zip(outs[r], ref):
            assert np.array_equal(a, b), r
        a, b = (os.path.join("outputs", p + cfg["output_prefix"], "metrics.csv") for p in ("", "seq_"))
        assert open(a, "rb").read() == open(b, "rb").read(), r
    assert kmc_simulation.last_run_info["beam"]["updates"] == 7


def test_refused_combinations(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    base = dict(L=8, n_steps=5, thermal_scheme="implicit", laser=dict(power=1.0, path=dict(pattern="line", speed=1.0)))
    for kw, word in ((dict(thermal_scheme="explicit"), "thermal_scheme='implicit'"), (dict(mode="B", box=8, thermal_scheme="explicit"), "mode 'A'"),
                     (dict(thermal_updates=False), "thermal_updates"), (dict(checkpoint_every=2), "checkpoint"),
                     (dict(laser=dict(power=1.0, path=dict(pattern="zigzag", speed=1.0))), "pattern"),
                     (dict(laser=dict(power=1.0, path=dict(speed=1.0))), "path"),
                     (dict(laser=dict(path=dict(pattern="line", speed=1.0))), "missing"),
                     (dict(laser=dict(power=1.0, start=0.0, path=dict(pattern="line", speed=1.0))), "unknown keys"),
                     (dict(laser=dict(power=1.0, path=dict(pattern="raster", speed=1.0))), "hatch")):
        with pytest.raises(ValueError) as err:
            kmc_simulation.run_kmc(**{**base, **kw})
        assert word in str(err.value), (word, str(err.value))
    ens = kmc_simulation.run_kmc_ensemble
    with pytest.raises(ValueError, match="thermal_scheme='implicit'"):
        ens([dict(output_prefix="a", laser=base["laser"])], 8, 5)
    with pytest.raises(ValueError, match="'path'"):
        ens([dict(output_prefix="a", laser=base["laser"]), dict(output_prefix="b", laser=dict(power=1.0, start=0.0, speed=1.0))], 8, 5,
            thermal_scheme="implicit")
    with pytest.raises(ValueError, match="depth"):
        ens([dict(output_prefix="a", laser=base["laser"]), dict(output_prefix="b", laser=dict(base["laser"], depth=2))], 8, 5, thermal_scheme="implicit")


def test_driver_flags(tmp_path, monkeypatch, capsys):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["main.py", "--L", "12", "--steps", "45", "--levels", "0.1", "--thermal-scheme", "implicit", "--laser-power", "2.0",
                                      "--scan", "raster", "--scan-speed", "3", "--hatch", "4", "--beam-depth", "2", "--penetration", "1e-5"])
    runpy.run_module("main", run_name="__main__")
    assert os.path.exists("outputs/impurity_c_10/metrics.csv")
    info = kmc_simulation.last_run_info["beam"]
    assert info["path"] == dict(pattern="raster", speed=3.0, hatch=4.0) and info["depth"] == 2 and info["updates"] == 3
    monkeypatch.setattr(sys, "argv", ["gv_sweep.py", "--L", "12", "--steps", "45", "--temps", "2800", "--nu-dep", "2e13", "--carbon", "0.1",
                                      "--thermal-scheme", "implicit", "--laser-power", "2.0", "--scan-speed", "3", "--scan", "serpentine", "--hatch", "4",
                                      "--beam-depth", "3"])
    runpy.run_module("gv_sweep", run_name="__main__")
    info = kmc_simulation.last_run_info["beam"]
    assert info["path"] == dict(pattern="serpentine", speed=3.0, hatch=4.0) and info["depth"] == 3
    assert list(pd.read_csv("outputs/gv_sweep/gv_map.csv")["power"]) == [2.0]
    import main as main_mod
    with pytest.raises(ValueError, match="--laser-power"):
        main_mod.main(12, 5, (0.1,), thermal_scheme="implicit", scan="line")
    with pytest.raises(ValueError, match="--scan"):
        main_mod.main(12, 5, (0.1,), hatch=3.0)
    capsys.readouterr()
