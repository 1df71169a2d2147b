"""The grain columns in the product layer: run_kmc(grain_metrics=True) in both modes (alone, with a laser and behind the
texture columns), grains.csv, run_kmc_ensemble(grain_metrics=True) against the sequential runs, and gv_sweep's --grains
columns.  The columns of the last row are compared with metrics.grain_metrics of the NumPy comparator (grain_ref.py) on the
lattice the run returns, clustered on a fresh handle; without the option the files are the ones a run without it writes."""
import csv
import os

import numpy as np
import pandas as pd
import pytest

import grain_ref as GR

pytestmark = pytest.mark.gpu

L, N_STEPS, EVERY = 12, 250, 80
BASE18 = ["Step", "Time", "AspectRatio", "EquiaxedFraction", "NucleationDensity", "DefectDensity", "AvgGrainSize", "GrainCount",
          "W_Count", "Re_Count", "C_Count", "NucleationCount", "G_over_R", "G_phys", "R_phys", "G_over_R_phys", "CET_Class",
          "CET_Detected"]


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _want_final(state, theta, phi):
    """metrics.grain_metrics of the comparator on the final lattice (its clustering from a fresh handle)"""
    import cetkmc
    import metrics
    e = cetkmc.Engine(L)
    try:
        e.upload(state, theta, phi, np.full((L, L, L), 3000.0), np.zeros((L, L, L), np.int64))
        lab = e.clusters(0.5, labels=True)["labels"]
    finally:
        e.close()
    return metrics.grain_metrics(GR.grain_ref(lab, state, theta, phi))


def _check_last_row(prefix, want):
    import metrics
    df = pd.read_csv(f"outputs/{prefix}/metrics.csv", float_precision="round_trip")
    last = df.iloc[-1].to_dict()
    for k in metrics.GRAIN_COLUMNS:
        assert last[k] == want[k], (k, last[k], want[k])
    g = pd.read_csv(f"outputs/{prefix}/grains.csv", float_precision="round_trip")
    assert len(g) == int(last["GrainCount"]) == len(want["grains"]["id"]) and list(g.columns) == list(want["grains"])
    for k, v in want["grains"].items():
        assert np.array_equal(g[k].to_numpy(), v, equal_nan=True), k
    return df


@pytest.mark.parametrize("variant", ["A", "A_laser", "A_texture", "B"])
def test_run_kmc_grain_columns(variant, tmp_path, monkeypatch):
    import kmc_simulation
    import metrics
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, impurity_c=0.1, defect_fraction=0.01, metrics_every=EVERY)
    kw.update({"A": {}, "A_laser": dict(laser=dict(power=200.0, start=3.0, speed=0.5)), "A_texture": dict(texture_metrics=True),
               "B": dict(mode="B", box=L)}[variant])
    kmc_simulation.run_kmc(output_prefix="plain_0", **kw)
    state, _, _, theta, phi = kmc_simulation.run_kmc(output_prefix="gr_0", grain_metrics=True, **kw)
    plain, gr = _rows("outputs/plain_0/metrics.csv"), _rows("outputs/gr_0/metrics.csv")
    mid = list(metrics.TEXTURE_COLUMNS) if variant == "A_texture" else []
    assert plain[0] == BASE18 + mid and gr[0] == BASE18 + mid + list(metrics.GRAIN_COLUMNS)
    n0 = len(plain[0])
    assert len(plain) == len(gr) >= 4 and [r[:n0] for r in gr] == plain                  # the other columns: the same text
    assert sorted(os.listdir("outputs/plain_0")) == [f for f in sorted(os.listdir("outputs/gr_0")) if f != "grains.csv"]
    assert os.path.exists("outputs/gr_0/grains.csv")
    if mid:
        assert open("outputs/plain_0/texture.csv", "rb").read() == open("outputs/gr_0/texture.csv", "rb").read()
    df = _check_last_row("gr_0", _want_final(state, theta, phi))
    assert (df["Largest_grain_frac"] > 0).all() and (df["Grain_elong_mean"] >= 1.0).all()
    print(f"{variant}: elong {df['Grain_elong_mean'].tolist()} columnar {df['Columnar_vol_frac'].tolist()} "
          f"largest {df['Largest_grain_frac'].tolist()} same {df['Contact_same_frac'].tolist()}")


def test_ensemble_rows_equal_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    cfgs = [dict(impurity_c=0.05 * (r + 1), seed=42 + r, defect_fraction=0.01 * r, temp=2800 + 150 * r, output_prefix=f"e{r}_{r}")
            for r in range(3)]
    out = kmc_simulation.run_kmc_ensemble(cfgs, L, N_STEPS, rng="reference", metrics_every=EVERY, grain_metrics=True)
    for r, c in enumerate(cfgs):
        kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, metrics_every=EVERY, grain_metrics=True,
                               **dict(c, output_prefix="seq_" + c["output_prefix"]))
        for f in ("metrics.csv", "grains.csv"):
            a, b = (f"outputs/{p}{c['output_prefix']}/{f}" for p in ("", "seq_"))
            assert open(a, "rb").read() == open(b, "rb").read(), (c, f)
        state, _, _, theta, phi = out[r]
        _check_last_row(c["output_prefix"], _want_final(state, theta, phi))
    # without the option the ensemble's files have the 18 columns and no grains.csv, byte for byte the sequential run's
    kmc_simulation.run_kmc_ensemble([dict(cfgs[0], output_prefix="p0_0")], L, N_STEPS, metrics_every=EVERY)
    assert _rows("outputs/p0_0/metrics.csv")[0] == BASE18 and not os.path.exists("outputs/p0_0/grains.csv")
    seq = _rows("outputs/seq_e0_0/metrics.csv")
    assert [r[:18] for r in seq] == _rows("outputs/p0_0/metrics.csv")


def test_gv_sweep_grain_columns(tmp_path, monkeypatch):
    import gv_sweep
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, temps=(2800.0,), nu_deps=(2e13, 2e14), carbon=0.1)          # a 2 x 1 map
    m = gv_sweep.gv_sweep(grains=True, **kw)
    on_disk = pd.read_csv("outputs/gv_sweep/gv_map.csv", float_precision="round_trip")
    assert list(on_disk.columns) == list(m.columns) and len(m) == 2
    assert list(m.columns[-2:]) == ["Columnar_vol_frac", "Grain_elong_mean"]
    for q, v in enumerate(("2e+13", "2e+14")):
        last = pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/metrics.csv").iloc[-1]          # parsed as gv_sweep parses it
        assert m["Columnar_vol_frac"].iloc[q] == last["Columnar_vol_frac"] and m["Grain_elong_mean"].iloc[q] == last["Grain_elong_mean"]
        assert len(pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/grains.csv")) == int(last["GrainCount"])
    with_grains = open("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv", "rb").read()
    m0 = gv_sweep.gv_sweep(**kw)
    assert list(m0.columns) == ["T_sub", "nu_dep", "G_K_per_m", "V_m_per_s", "G_over_V", "AspectRatio", "EquiaxedFraction",
                                "GrainCount", "NucleationCount", "CET_Class", "CET_Detected"]
    assert m0.equals(m[list(m0.columns)])
    assert _rows("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv")[0] == BASE18
    assert len(with_grains) > len(open("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv", "rb").read())
