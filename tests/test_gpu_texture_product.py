"""The texture columns in the product layer: run_kmc(texture_metrics=True) alone and behind the layer columns, texture.csv,
run_kmc_ensemble(texture_metrics=True) against the sequential runs, and gv_sweep's --texture columns.  The columns of the last
row are compared with metrics.texture_metrics of the NumPy comparator (texture_ref.py) on the lattice the run returns,
clustered on a fresh handle; without the option the files are the ones a run without it writes."""
import csv
import os

import numpy as np
import pandas as pd
import pytest

import texture_ref as TR

pytestmark = pytest.mark.gpu

L, N_STEPS, EVERY = 12, 250, 80
BASE18 = ["Step", "Time", "AspectRatio", "EquiaxedFraction", "NucleationDensity", "DefectDensity", "AvgGrainSize", "GrainCount",
          "W_Count", "Re_Count", "C_Count", "NucleationCount", "G_over_R", "G_phys", "R_phys", "G_over_R_phys", "CET_Class",
          "CET_Detected"]


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


def _want_final(state, theta, phi):
    """metrics.texture_metrics of the comparator on the final lattice (its clustering from a fresh handle), at the
    product's settings: 36 bins, axis (1, 0, 0)"""
    import cetkmc
    import metrics
    from cetkmc.engine import texture_edges_deg
    e = cetkmc.Engine(L)
    try:
        e.upload(state, theta, phi, np.full((L, L, L), 3000.0), np.zeros((L, L, L), np.int64))
        lab = e.clusters(0.5, labels=True)["labels"]
    finally:
        e.close()
    ge, pe = TR.edges_cos(36, 180.0), TR.edges_cos(36, 90.0)
    values = (TR.face_values(lab, theta, phi), TR.pole_values(lab, theta, phi, (1.0, 0.0, 0.0)))
    assert TR.n_ambiguous(values, ge, pe) == 0
    prof = TR.texture_ref(lab, theta, phi, ge, pe, values=values)
    prof.update(gb_edges_deg=texture_edges_deg(36, 180.0), pole_edges_deg=texture_edges_deg(36, 90.0))
    return metrics.texture_metrics(prof)


def _check_last_row(prefix, want):
    import metrics
    df = pd.read_csv(f"outputs/{prefix}/metrics.csv", float_precision="round_trip")
    last = df.iloc[-1].to_dict()
    for k in metrics.TEXTURE_COLUMNS:
        assert last[k] == want[k], (k, last[k], want[k])
    tex = pd.read_csv(f"outputs/{prefix}/texture.csv", float_precision="round_trip")
    assert len(tex) == L and list(tex.columns) == list(want["planes"])
    for k, v in want["planes"].items():
        assert tex[k].tolist() == v.tolist(), k
    return df


@pytest.mark.parametrize("variant", ["A", "A_layers", "B"])
def test_run_kmc_texture_columns(variant, tmp_path, monkeypatch):
    import kmc_simulation
    import metrics
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, impurity_c=0.1, defect_fraction=0.01, metrics_every=EVERY)
    kw.update({"A": {}, "A_layers": dict(layer_metrics=True), "B": dict(mode="B", box=L)}[variant])
    kmc_simulation.run_kmc(output_prefix="plain_0", **kw)
    state, _, _, theta, phi = kmc_simulation.run_kmc(output_prefix="tex_0", texture_metrics=True, **kw)
    plain, tex = _rows("outputs/plain_0/metrics.csv"), _rows("outputs/tex_0/metrics.csv")
    mid = list(metrics.LAYER_COLUMNS) if variant == "A_layers" else []
    assert plain[0] == BASE18 + mid and tex[0] == BASE18 + mid + list(metrics.TEXTURE_COLUMNS)
    n0 = len(plain[0])
    assert len(plain) == len(tex) >= 4 and [r[:n0] for r in tex] == plain                # the other columns: the same text
    assert not os.path.exists("outputs/plain_0/texture.csv")
    if mid:
        assert open("outputs/plain_0/layers.csv", "rb").read() == open("outputs/tex_0/layers.csv", "rb").read()
    df = _check_last_row("tex_0", _want_final(state, theta, phi))
    assert (df["Pole_aligned_frac"] >= 0).all() and (df["Texture_bad"] == 0).all()
    print(f"{variant}: GB_faces {df['GB_faces'].tolist()} mean {df['GB_misorientation_mean_deg'].tolist()} "
          f"low {df['GB_low_angle_frac'].tolist()} pole {df['Pole_aligned_frac'].tolist()}")


def test_ensemble_rows_equal_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    cfgs = [dict(impurity_c=0.05 * (r + 1), seed=42 + r, defect_fraction=0.01 * r, temp=2800 + 150 * r, output_prefix=f"e{r}_{r}")
            for r in range(3)]
    out = kmc_simulation.run_kmc_ensemble(cfgs, L, N_STEPS, rng="reference", metrics_every=EVERY, texture_metrics=True)
    for r, c in enumerate(cfgs):
        kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, metrics_every=EVERY, texture_metrics=True,
                               **dict(c, output_prefix="seq_" + c["output_prefix"]))
        for f in ("metrics.csv", "texture.csv"):
            a, b = (f"outputs/{p}{c['output_prefix']}/{f}" for p in ("", "seq_"))
            assert open(a, "rb").read() == open(b, "rb").read(), (c, f)
        state, _, _, theta, phi = out[r]
        _check_last_row(c["output_prefix"], _want_final(state, theta, phi))
    # without the option the ensemble's files have the 18 columns and no texture.csv, byte for byte the sequential run's
    kmc_simulation.run_kmc_ensemble([dict(cfgs[0], output_prefix="p0_0")], L, N_STEPS, metrics_every=EVERY)
    assert _rows("outputs/p0_0/metrics.csv")[0] == BASE18 and not os.path.exists("outputs/p0_0/texture.csv")
    seq = _rows("outputs/seq_e0_0/metrics.csv")
    assert [r[:18] for r in seq] == _rows("outputs/p0_0/metrics.csv")


def test_gv_sweep_texture_columns(tmp_path, monkeypatch):
    import gv_sweep
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, temps=(2800.0,), nu_deps=(2e13, 2e14), carbon=0.1)          # a 2 x 1 map
    m = gv_sweep.gv_sweep(texture=True, **kw)
    on_disk = pd.read_csv("outputs/gv_sweep/gv_map.csv", float_precision="round_trip")
    assert list(on_disk.columns) == list(m.columns) and len(m) == 2
    assert list(m.columns[-2:]) == ["GB_low_angle_frac", "Pole_aligned_frac"]
    for q, v in enumerate(("2e+13", "2e+14")):
        last = pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/metrics.csv").iloc[-1]          # parsed as gv_sweep parses it
        assert m["GB_low_angle_frac"].iloc[q] == last["GB_low_angle_frac"] and m["Pole_aligned_frac"].iloc[q] == last["Pole_aligned_frac"]
        assert len(pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/texture.csv")) == L
    textured = open("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv", "rb").read()
    m0 = gv_sweep.gv_sweep(**kw)
    assert list(m0.columns) == ["T_sub", "nu_dep", "G_K_per_m", "V_m_per_s", "G_over_V", "AspectRatio", "EquiaxedFraction",
                                "GrainCount", "NucleationCount", "CET_Class", "CET_Detected"]
    assert m0.equals(m[list(m0.columns)])
    assert _rows("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv")[0] == BASE18
    assert len(textured) > len(open("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv", "rb").read())
