"""The implicit scheme in the product layer: run_kmc(laser=..., thermal_scheme="implicit") repeatable and reported in
last_run_info, a resume bit-identical, thermal_scheme="explicit" = the call without the keyword file by file, the pure-function
drop-ins' ``scheme`` keyword against the comparator, run_kmc_ensemble with one shared value against sequential run_kmc calls,
the refused combinations and the two driver flags."""
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


def test_run_kmc_laser_implicit_repeatable(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    a = kmc_simulation.run_kmc(laser=LASER, thermal_scheme="implicit", output_prefix="a_0", **KW)
    assert kmc_simulation.last_run_info["thermal_scheme"] == "implicit" and kmc_simulation.last_run_info["thermal_substeps"] == 1
    b = kmc_simulation.run_kmc(laser=LASER, remelt=True, thermal_substeps=3, thermal_scheme="implicit", output_prefix="b_0", **KW)
    assert kmc_simulation.last_run_info["thermal_substeps"] == 3
    c = kmc_simulation.run_kmc(laser=LASER, thermal_scheme="implicit", output_prefix="c_0", **KW)
    for x, y in zip(a, c):
        assert np.array_equal(x, y)
    assert _files("a_0") == _files("c_0")
    assert list(pd.read_csv("outputs/b_0/metrics.csv").columns[-2:]) == ["RemeltPasses", "RemeltedVoxels"]      # with remelt as well
    assert len(b) == len(a)
    # the implicit field is another field: the run differs from the one with the reference's single explicit step
    plain = kmc_simulation.run_kmc(laser=LASER, output_prefix="plain_0", **KW)
    assert kmc_simulation.last_run_info["thermal_scheme"] == "explicit"
    assert open("outputs/plain_0/metrics.csv", "rb").read() != open("outputs/a_0/metrics.csv", "rb").read()
    assert len(plain) == len(a)


def test_explicit_is_the_call_without_the_keyword(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(KW, laser=LASER, front_metrics=True, solid_metrics=True)
    a = kmc_simulation.run_kmc(output_prefix="x_0", **kw)
    files_a = _files("x_0")
    os.rename("outputs/x_0", "outputs/kept_0")
    b = kmc_simulation.run_kmc(thermal_scheme="explicit", output_prefix="x_0", **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert _files("x_0") == files_a and len(files_a) >= 3
    # ... and so is its checkpoint: no new key
    kmc_simulation.run_kmc(output_prefix="ck_0", checkpoint_every=51, thermal_scheme="explicit", **dict(KW, n_steps=51))
    assert "thermal_scheme" not in kmc_simulation.load_checkpoint("outputs/ck_0/checkpoint.npz")["extra"]


def test_resume_is_bit_identical(tmp_path, monkeypatch):
    """no laser (a checkpoint does not carry prev_state)"""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(KW, thermal_scheme="implicit")
    whole = kmc_simulation.run_kmc(output_prefix="whole_0", **kw)
    # the first part ends on a metrics step (50), so that it writes no row the whole run does not have
    kmc_simulation.run_kmc(output_prefix="part_0", checkpoint_every=51, **dict(kw, n_steps=51))
    assert kmc_simulation.load_checkpoint("outputs/part_0/checkpoint.npz")["extra"]["thermal_scheme"] == "implicit"
    rest = kmc_simulation.run_kmc(output_prefix="part_0", resume_from="outputs/part_0/checkpoint.npz", **kw)
    for x, y in zip(whole, rest):
        assert np.array_equal(x, y)
    assert open("outputs/whole_0/metrics.csv", "rb").read() == open("outputs/part_0/metrics.csv", "rb").read()
    with pytest.raises(ValueError, match="thermal_scheme"):             # the checkpoint carries the setting
        kmc_simulation.run_kmc(output_prefix="part_0", resume_from="outputs/part_0/checkpoint.npz", **dict(kw, thermal_scheme="explicit"))


def test_drop_in_updates_with_scheme(oracle_mod):
    """thermal_solver.update_temperature / update_temperature_cet(scheme="implicit") against the comparator; the cached handle
    is back at the explicit scheme afterwards"""
    import implicit_cases as ic
    import implicit_ref
    import substep_ref
    import thermal_solver
    L, n = 25, 2
    (state, _th, _ph, T, _df), prev, _q = ic.direct_fields(L)
    try:
        for mode in (1, 2):
            lat = oracle_mod.Lattice(state, np.zeros_like(T), np.zeros_like(T), T, impurity_c=0.0)
            lat.prev_state = np.ascontiguousarray(prev, np.int8)
            q = oracle_mod.laser_source_plane(L, (L - 1, 3.0), 60.0)
            implicit_ref.update(lat, n, 1e-6, mode, q, use_latent=True, scrub=False)
            if mode == 1:
                got = thermal_solver.update_temperature_cet(T, state, 1e-6, substeps=n, scheme="implicit")
                one = thermal_solver.update_temperature_cet(T, state, 1e-6)
            else:
                got = thermal_solver.update_temperature(T, state, prev, 1e-6, (L - 1, 3.0), 60.0, substeps=n, scheme="implicit")
                one = thermal_solver.update_temperature(T, state, prev, 1e-6, (L - 1, 3.0), 60.0)
            assert got.tobytes() == lat.T.tobytes(), mode
            ref = oracle_mod.Lattice(state, np.zeros_like(T), np.zeros_like(T), T, impurity_c=0.0)
            ref.prev_state = np.ascontiguousarray(prev, np.int8)
            substep_ref.update(ref, 1, 1e-6, mode, q, use_latent=True, scrub=False)
            assert one.tobytes() == ref.T.tobytes(), mode
        for bad in ("Implicit", 1, None):
            with pytest.raises(ValueError, match="scheme"):
                thermal_solver.update_temperature_cet(T, state, 1e-6, scheme=bad)
    finally:
        thermal_solver.close_engines()


def test_ensemble_vs_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, n = 16, 130
    cfgs = [dict(impurity_c=0.1, seed=42 + s, defect_fraction=3e-3, output_prefix=f"e{s}_{s}",
                 laser=dict(power=100.0 + 30.0 * s, start=4.0, speed=0.5)) for s in range(3)]
    outs = kmc_simulation.run_kmc_ensemble(cfgs, L, n, metrics_every=50, thermal_scheme="implicit")
    infos = list(kmc_simulation.last_ensemble_info)
    for r, cfg in enumerate(cfgs):
        ref = kmc_simulation.run_kmc(L=L, n_steps=n, metrics_every=50, thermal_scheme="implicit", **dict(cfg, output_prefix="seq_" + cfg["output_prefix"]))
        for a, b in zip(outs[r], ref):
            assert np.array_equal(a, b), r
        a, b = (os.path.join("outputs", p + cfg["output_prefix"], "metrics.csv") for p in ("", "seq_"))
        assert open(a, "rb").read() == open(b, "rb").read(), r
        assert infos[r]["thermal_scheme"] == "implicit" == kmc_simulation.last_run_info["thermal_scheme"]


def test_refused_combinations(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    for kw in (dict(mode="B", box=8), dict(thermal_updates=False), dict(thermal_scheme="Implicit"), dict(thermal_scheme=1),
               dict(thermal_scheme=None)):
        with pytest.raises(ValueError, match="thermal_scheme"):
            kmc_simulation.run_kmc(**{**dict(L=8, n_steps=5, thermal_scheme="implicit"), **kw})
    ens = kmc_simulation.run_kmc_ensemble
    with pytest.raises(ValueError, match="thermal_scheme='implicit' needs rng='reference'"):
        ens([dict(output_prefix="a")], 8, 5, rng="counter", thermal_scheme="implicit")
    with pytest.raises(ValueError, match="thermal_scheme='implicit' needs mode 'A'"):
        kmc_simulation.run_kmc(L=8, n_steps=5, thermal_scheme="implicit", mode="B", box=8)
    with pytest.raises(ValueError, match="thermal_scheme"):
        ens([dict(output_prefix="a")], 8, 5, thermal_updates=False, thermal_scheme="implicit")
    with pytest.raises(ValueError, match="thermal_scheme"):
        ens([dict(output_prefix="a")], 8, 5, thermal_scheme="adi")
    assert not os.path.exists("outputs")                                 # refused before anything ran


def test_driver_flags(tmp_path, monkeypatch, capsys):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["gv_sweep.py", "--L", "12", "--steps", "60", "--temps", "2800", "--nu-dep", "2e13", "--carbon", "0.1",
                                      "--laser-power", "150", "--scan-speed", "0.5", "--thermal-scheme", "implicit"])
    runpy.run_module("gv_sweep", run_name="__main__")
    assert os.path.exists("outputs/gv_sweep/T2800_V2e+13_P150_S0.5_c_10/metrics.csv")
    assert kmc_simulation.last_run_info["thermal_scheme"] == "implicit"
    monkeypatch.setattr(sys, "argv", ["main.py", "--L", "12", "--steps", "45", "--levels", "0.1", "--thermal-scheme", "implicit",
                                      "--thermal-substeps", "2"])
    runpy.run_module("main", run_name="__main__")
    assert os.path.exists("outputs/impurity_c_10/metrics.csv")
    assert kmc_simulation.last_run_info["thermal_scheme"] == "implicit" and kmc_simulation.last_run_info["thermal_substeps"] == 2
    capsys.readouterr()
