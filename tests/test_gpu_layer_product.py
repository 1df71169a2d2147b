"""The layer columns in the product layer: run_kmc(layer_metrics=True) in mode A, mode A with a laser and mode B, alone and
together with front_metrics (column order), layers.csv, run_kmc_ensemble(layer_metrics=True) against the sequential runs, and
the layer columns of gv_sweep's map.  The columns of the last row are compared with metrics.layer_metrics of the NumPy
comparator (layer_ref.py) on the lattice the run returns, clustered on a fresh handle."""
import csv

import numpy as np
import pandas as pd
import pytest

import layer_ref as LR

pytestmark = pytest.mark.gpu

L, N_STEPS, EVERY = 16, 330, 80
LASER = dict(power=150.0, start=2.0, speed=0.5)
BASE18 = ["Step", "Time", "AspectRatio", "EquiaxedFraction", "NucleationDensity", "DefectDensity", "AvgGrainSize", "GrainCount",
          "W_Count", "Re_Count", "C_Count", "NucleationCount", "G_over_R", "G_phys", "R_phys", "G_over_R_phys", "CET_Class",
          "CET_Detected"]


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _want_final(state, theta, phi):
    """metrics.layer_metrics of the comparator on the final lattice (its clustering from a fresh handle)"""
    import cetkmc
    import metrics
    from constants import CET_AR_THRESHOLD, VOXEL_SIZE
    e = cetkmc.Engine(L)
    try:
        e.upload(state, theta, phi, np.full((L, L, L), 3000.0), np.zeros((L, L, L), np.int64))
        cl = e.clusters(0.5, labels=True)
    finally:
        e.close()
    return metrics.layer_metrics(LR.layer_ref(cl["labels"], state, cl["bbox"], cl["first"], CET_AR_THRESHOLD), L, VOXEL_SIZE)


def _check_last_row(prefix, want):
    import metrics
    df = pd.read_csv(f"outputs/{prefix}/metrics.csv", float_precision="round_trip")
    last = df.iloc[-1].to_dict()
    assert int(last["CET_plane"]) == want["CET_plane"]
    for k in metrics.LAYER_COLUMNS[1:]:
        assert last[k] == want[k], (k, last[k], want[k])
    lay = pd.read_csv(f"outputs/{prefix}/layers.csv", float_precision="round_trip")
    assert len(lay) == L and list(lay.columns) == list(want["planes"])
    for k, v in want["planes"].items():
        assert lay[k].tolist() == v.tolist(), k
    return df


@pytest.mark.parametrize("variant", ["A", "A_laser", "B", "A_front", "A_laser_front"])
def test_run_kmc_layer_columns(variant, tmp_path, monkeypatch):
    import kmc_simulation
    import metrics
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, impurity_c=0.1, defect_fraction=0.01, metrics_every=EVERY)
    front = variant.endswith("_front")
    kw.update({"A": {}, "A_laser": dict(laser=LASER), "B": dict(mode="B", box=L)}[variant[:-6] if front else variant])
    if front:
        kw["front_metrics"] = True
    kmc_simulation.run_kmc(output_prefix="plain_0", **kw)
    state, _, _, theta, phi = kmc_simulation.run_kmc(output_prefix="layer_0", layer_metrics=True, **kw)
    plain, layer = _rows("outputs/plain_0/metrics.csv"), _rows("outputs/layer_0/metrics.csv")
    mid = (list(metrics.FRONT_COLUMNS) + ["V_front"]) if front else []
    assert plain[0] == BASE18 + mid and layer[0] == BASE18 + mid + list(metrics.LAYER_COLUMNS)
    n0 = len(plain[0])
    assert len(plain) == len(layer) >= 5 and [r[:n0] for r in layer] == plain            # the other columns: the same text
    df = _check_last_row("layer_0", _want_final(state, theta, phi))
    assert (df["Intercept_build_um"] > 0).all()                    # every row has occupied voxels
    print(f"{variant}: CET_plane {df['CET_plane'].tolist()} EqAreaFrac {df['EqAreaFrac'].tolist()} "
          f"InterceptRatio {df['InterceptRatio'].tolist()} GB_frac_C {df['GB_frac_C'].tolist()}")


def test_ensemble_rows_equal_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    cfgs = [dict(impurity_c=0.05 * (r + 1), seed=42 + r, defect_fraction=0.01 * r, temp=2800 + 150 * r, output_prefix=f"e{r}_{r}")
            for r in range(3)]
    kmc_simulation.run_kmc_ensemble(cfgs, L, N_STEPS, rng="reference", metrics_every=EVERY, layer_metrics=True)
    for c in cfgs:
        kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, metrics_every=EVERY, layer_metrics=True,
                               **dict(c, output_prefix="seq_" + c["output_prefix"]))
        for f in ("metrics.csv", "layers.csv"):
            a, b = (f"outputs/{p}{c['output_prefix']}/{f}" for p in ("", "seq_"))
            assert open(a, "rb").read() == open(b, "rb").read(), (c, f)
        assert "InterceptRatio" in pd.read_csv(a.replace("layers.csv", "metrics.csv")).columns
    # without the option the ensemble's files have the 18 columns and no layers.csv
    import os
    kmc_simulation.run_kmc_ensemble([dict(cfgs[0], output_prefix="p0_0")], L, 60, metrics_every=EVERY)
    assert _rows("outputs/p0_0/metrics.csv")[0] == BASE18 and not os.path.exists("outputs/p0_0/layers.csv")


def test_gv_sweep_layer_columns(tmp_path, monkeypatch):
    import gv_sweep
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, temps=(2800.0,), nu_deps=(2e13, 2e14), carbon=0.1)
    m = gv_sweep.gv_sweep(layers=True, **kw)
    on_disk = pd.read_csv("outputs/gv_sweep/gv_map.csv", float_precision="round_trip")
    assert list(on_disk.columns) == list(m.columns) and len(m) == 2
    assert list(m.columns[-2:]) == ["CET_height_um", "InterceptRatio"]
    for q, v in enumerate(("2e+13", "2e+14")):
        last = pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/metrics.csv", float_precision="round_trip").iloc[-1]
        assert m["CET_height_um"].iloc[q] == last["CET_height_um"] and m["InterceptRatio"].iloc[q] == last["InterceptRatio"]
        assert len(pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/layers.csv")) == L
    mf = gv_sweep.gv_sweep(layers=True, front=True, **kw)
    assert list(mf.columns[-5:]) == ["G_front_K_per_m", "V_front_m_per_s", "G_over_V_front", "CET_height_um", "InterceptRatio"]
    m0 = gv_sweep.gv_sweep(**kw)
    assert list(m0.columns) == ["T_sub", "nu_dep", "G_K_per_m", "V_m_per_s", "G_over_V", "AspectRatio", "EquiaxedFraction",
                                "GrainCount", "NucleationCount", "CET_Class", "CET_Detected"]
    assert _rows("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv")[0] == BASE18
