"""Thermal boundaries in the product layer: run_kmc(thermal_scheme="implicit",
thermal_boundary="gradient") repeatable, reported in last_run_info and holding the run's initial ramp; ``laser=`` with the
substrate sink; a resume bit-identical; the keyword absent = the call with thermal_boundary=None file by file; the pure-function
drop-ins' ``boundary`` keyword against the comparator; run_kmc_ensemble with one shared value against sequential run_kmc calls;
the refused combinations and the three driver flags."""
import os
import runpy
import sys

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

LASER = dict(power=150.0, start=2.0, speed=0.5)
KW = dict(L=24, n_steps=130, impurity_c=0.1, defect_fraction=3e-3, metrics_every=50, thermal_scheme="implicit")


def _files(prefix):
    d = os.path.join("outputs", prefix)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if os.path.isfile(os.path.join(d, f))}


def _sink():
    import thermal_solver
    from constants import T_SUB
    return thermal_solver.thermal_boundary(bottom=("fixed", T_SUB))


def test_gradient_is_repeatable_and_holds_the_ramp(tmp_path, monkeypatch):
    """L = 24, 101 steps (six updates), the field read from the checkpoint at the end: within 1e-9 K of the initial ramp wherever
    no clip value was reached; the same run between insulated walls is more than 1 K off"""
    import kmc_simulation
    from constants import T_MELT, T_SUB
    from lattice_init import initialize_lattice
    monkeypatch.chdir(tmp_path)
    kw = dict(KW, n_steps=101, checkpoint_every=101)
    a = kmc_simulation.run_kmc(thermal_boundary="gradient", output_prefix="a_0", **kw)
    info = kmc_simulation.last_run_info["thermal_boundary"]
    assert info == kmc_simulation.run_gradient_boundary(24) and info["beta"] == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0]
    b = kmc_simulation.run_kmc(thermal_boundary="gradient", output_prefix="b_0", **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    fa, fb = _files("a_0"), _files("b_0")
    assert fa.keys() == fb.keys() and all(fa[f] == fb[f] for f in fa if f != "checkpoint.npz")
    T0 = initialize_lattice(lattice_size=24, n_seeds=5, T_sub=T_SUB, impurity_c=0.1)[3]
    Ta = kmc_simulation.load_checkpoint("outputs/a_0/checkpoint.npz")["T"]
    assert Ta.tobytes() == kmc_simulation.load_checkpoint("outputs/b_0/checkpoint.npz")["T"].tobytes()
    free = kmc_simulation.run_kmc(output_prefix="free_0", **kw)
    assert kmc_simulation.last_run_info["thermal_boundary"] is None and len(free) == len(a)
    Tf = kmc_simulation.load_checkpoint("outputs/free_0/checkpoint.npz")["T"]
    inside = (Ta != T_SUB) & (Ta != 1.1 * T_MELT)
    print("held:", np.abs(Ta - T0)[inside].max(), "insulated:", np.abs(Tf - T0).max(), "voxels off the clip values:", int(inside.sum()))
    assert inside.sum() > 0.9 * inside.size
    assert np.abs(Ta - T0)[inside].max() <= 1e-9
    assert np.abs(Tf - T0).max() > 1.0


def test_laser_with_the_sink(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(KW, laser=LASER, thermal_scheme="implicit")
    a = kmc_simulation.run_kmc(thermal_boundary=_sink(), output_prefix="a_0", **kw)
    assert kmc_simulation.last_run_info["thermal_boundary"] == _sink()
    c = kmc_simulation.run_kmc(thermal_boundary=_sink(), remelt=True, thermal_substeps=3, output_prefix="c_0", **kw)
    assert list(pd.read_csv("outputs/c_0/metrics.csv").columns[-2:]) == ["RemeltPasses", "RemeltedVoxels"] and len(c) == len(a)
    b = kmc_simulation.run_kmc(thermal_boundary=_sink(), output_prefix="b_0", **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert _files("a_0") == _files("b_0")


def test_keyword_absent_is_none_and_checkpoints_carry_no_key(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(KW, laser=LASER, front_metrics=True, solid_metrics=True)
    a = kmc_simulation.run_kmc(output_prefix="x_0", **kw)
    files_a = _files("x_0")
    os.rename("outputs/x_0", "outputs/kept_0")
    b = kmc_simulation.run_kmc(thermal_boundary=None, output_prefix="x_0", **kw)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert _files("x_0") == files_a and len(files_a) >= 3
    kmc_simulation.run_kmc(output_prefix="ck_0", checkpoint_every=51, **dict(KW, n_steps=51))
    assert "thermal_bc" not in kmc_simulation.load_checkpoint("outputs/ck_0/checkpoint.npz")["extra"]


def test_resume_is_bit_identical(tmp_path, monkeypatch):
    """a cooling rate, so that the face temperatures depend on the global step across the resume"""
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    bnd = kmc_simulation.run_gradient_boundary(24, cooling_rate=1e8)
    assert bnd["ramp"][4:] == [-100.0, -100.0]
    kw = dict(KW, thermal_boundary=bnd)
    whole = kmc_simulation.run_kmc(output_prefix="whole_0", **kw)
    kmc_simulation.run_kmc(output_prefix="part_0", checkpoint_every=51, **dict(kw, n_steps=51))
    assert kmc_simulation.load_checkpoint("outputs/part_0/checkpoint.npz")["extra"]["thermal_bc"] == bnd
    rest = kmc_simulation.run_kmc(output_prefix="part_0", resume_from="outputs/part_0/checkpoint.npz", **kw)
    for x, y in zip(whole, rest):
        assert np.array_equal(x, y)
    assert open("outputs/whole_0/metrics.csv", "rb").read() == open("outputs/part_0/metrics.csv", "rb").read()
    for other in (None, "gradient"):
        with pytest.raises(ValueError, match="thermal_boundary"):            # the checkpoint carries the setting
            kmc_simulation.run_kmc(output_prefix="part_0", resume_from="outputs/part_0/checkpoint.npz", **dict(kw, thermal_boundary=other))


def test_drop_in_updates_with_boundary(oracle_mod):
    """thermal_solver.update_temperature / update_temperature_cet(scheme="implicit", boundary=...) against the comparator; the
    cached handle is back at the adiabatic explicit update afterwards"""
    import boundary_ref as br
    import implicit_cases as ic
    import substep_ref
    import thermal_solver
    L, n = 25, 2
    (state, _th, _ph, T, _df), prev, _q = ic.direct_fields(L)
    bnd = thermal_solver.thermal_boundary(bottom=("fixed", 2800.0), top=("convective", 3.0e7, 300.0), sides=("convective", 1.0e7, 3500.0))
    ref_b = br.boundary(bnd["beta"], bnd["T_ext"], bnd["ramp"])
    assert 0.0 < bnd["beta"][2] < bnd["beta"][1] < 1.0
    try:
        for mode in (1, 2):
            lat = oracle_mod.Lattice(state, np.zeros_like(T), np.zeros_like(T), T, impurity_c=0.0)
            lat.prev_state = np.ascontiguousarray(prev, np.int8)
            q = oracle_mod.laser_source_plane(L, (L - 1, 3.0), 60.0)
            br.update(lat, n, 1e-6, mode, q, use_latent=True, scrub=False, bc=ref_b, u=0)
            if mode == 1:
                got = thermal_solver.update_temperature_cet(T, state, 1e-6, substeps=n, scheme="implicit", boundary=bnd)
                one = thermal_solver.update_temperature_cet(T, state, 1e-6)
            else:
                got = thermal_solver.update_temperature(T, state, prev, 1e-6, (L - 1, 3.0), 60.0, substeps=n, scheme="implicit", boundary=bnd)
                one = thermal_solver.update_temperature(T, state, prev, 1e-6, (L - 1, 3.0), 60.0)
            assert got.tobytes() == lat.T.tobytes(), mode
            ref = oracle_mod.Lattice(state, np.zeros_like(T), np.zeros_like(T), T, impurity_c=0.0)
            ref.prev_state = np.ascontiguousarray(prev, np.int8)
            substep_ref.update(ref, 1, 1e-6, mode, q, use_latent=True, scrub=False)
            assert one.tobytes() == ref.T.tobytes(), mode
        with pytest.raises(ValueError, match="implicit"):
            thermal_solver.update_temperature_cet(T, state, 1e-6, boundary=bnd)
    finally:
        thermal_solver.close_engines()


def test_ensemble_vs_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, n = 16, 130
    bnd = dict(_sink(), ramp=[-20.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    cfgs = [dict(impurity_c=0.1, seed=42 + s, defect_fraction=3e-3, output_prefix=f"e{s}_{s}",
                 laser=dict(power=100.0 + 30.0 * s, start=4.0, speed=0.5)) for s in range(3)]
    outs = kmc_simulation.run_kmc_ensemble(cfgs, L, n, metrics_every=50, thermal_scheme="implicit", thermal_boundary=bnd)
    infos = list(kmc_simulation.last_ensemble_info)
    for r, cfg in enumerate(cfgs):
        ref = kmc_simulation.run_kmc(L=L, n_steps=n, metrics_every=50, thermal_scheme="implicit", thermal_boundary=bnd,
                                     **dict(cfg, output_prefix="seq_" + cfg["output_prefix"]))
        for a, b in zip(outs[r], ref):
            assert np.array_equal(a, b), r
        a, b = (os.path.join("outputs", p + cfg["output_prefix"], "metrics.csv") for p in ("", "seq_"))
        assert open(a, "rb").read() == open(b, "rb").read(), r
        assert infos[r]["thermal_boundary"] == bnd == kmc_simulation.last_run_info["thermal_boundary"]
    plain = kmc_simulation.run_kmc(L=L, n_steps=n, metrics_every=50, thermal_scheme="implicit", **dict(cfgs[0], output_prefix="plain_0"))
    assert len(plain) == len(outs[0])


def test_refused_combinations(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    base = dict(L=8, n_steps=5, thermal_scheme="implicit", thermal_boundary="gradient")
    for kw, word in ((dict(mode="B", box=8, thermal_scheme="explicit"), "mode 'A'"), (dict(thermal_scheme="explicit"), "thermal_scheme='implicit'"),
                     (dict(thermal_boundary="sink"), "must be None"), (dict(thermal_boundary=dict(beta=[1.0] * 5)), "must be None"),
                     (dict(thermal_boundary=3), "must be None")):
        with pytest.raises(ValueError, match="thermal_boundary") as err:
            kmc_simulation.run_kmc(**{**base, **kw})
        assert word in str(err.value), (word, str(err.value))
    with pytest.raises(ValueError):                       # (thermal_scheme='implicit' itself needs thermal_updates)
        kmc_simulation.run_kmc(**dict(base, thermal_updates=False))
    with pytest.raises(ValueError, match="thermal_boundary needs thermal_updates=True"):
        kmc_simulation._thermal_boundary("gradient", 8, 2800.0, True, "implicit", False)
    ens = kmc_simulation.run_kmc_ensemble
    with pytest.raises(ValueError, match="thermal_boundary"):
        ens([dict(output_prefix="a")], 8, 5, thermal_boundary="gradient")
    with pytest.raises(ValueError, match="one temp"):
        ens([dict(output_prefix="a", temp=2800.0), dict(output_prefix="b", temp=3000.0)], 8, 5, thermal_scheme="implicit", thermal_boundary="gradient")
    assert not os.path.exists("outputs")                                 # refused before anything ran


def test_driver_flags(tmp_path, monkeypatch, capsys):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sys, "argv", ["gv_sweep.py", "--L", "12", "--steps", "60", "--temps", "2800", "--nu-dep", "2e13", "--carbon", "0.1",
                                      "--thermal-scheme", "implicit", "--hold-gradient", "--cooling-rate", "1e6"])
    runpy.run_module("gv_sweep", run_name="__main__")
    assert kmc_simulation.last_run_info["thermal_boundary"] == kmc_simulation.run_gradient_boundary(12, 2800.0, 1e6)
    table = pd.read_csv("outputs/gv_sweep/gv_map.csv")
    assert list(table.columns[2:6]) == ["G_K_per_m", "V_m_per_s", "G_over_V", "CoolingRate_K_per_s"] and table["CoolingRate_K_per_s"][0] == 1e6
    monkeypatch.setattr(sys, "argv", ["gv_sweep.py", "--L", "12", "--steps", "60", "--temps", "2800", "--nu-dep", "2e13", "--carbon", "0.1"])
    runpy.run_module("gv_sweep", run_name="__main__")
    assert "CoolingRate_K_per_s" not in pd.read_csv("outputs/gv_sweep/gv_map.csv").columns       # without the flag: the table of before
    for flag, want in (("gradient", kmc_simulation.run_gradient_boundary(12)), ("sink", _sink())):
        monkeypatch.setattr(sys, "argv", ["main.py", "--L", "12", "--steps", "45", "--levels", "0.1", "--thermal-scheme", "implicit",
                                          "--thermal-boundary", flag])
        runpy.run_module("main", run_name="__main__")
        assert os.path.exists("outputs/impurity_c_10/metrics.csv")
        assert kmc_simulation.last_run_info["thermal_boundary"] == want
    capsys.readouterr()
