"""The build product (run_kmc(build=...)) at L = 16 and L = 24, three layers.

A run is repeatable bit for bit, with and without a laser path.  It equals the same run with ``Engine.shift`` replaced by
the host route -- download, the comparator tests/shift_ref.py, upload -- in the fields it returns, in metrics.csv and in where it
leaves both host generators (layer_metrics alone: the host route cannot carry the maps).  build_layers.csv reaches through the
whole part, L + (N - 1) h planes with contiguous BuildHeight, and the planes a layer retires carry the records of that layer's
last metrics row.  Without a build metrics.csv is, byte for byte, the file the parent commit's run_kmc wrote at the same arguments
(tests/golden/shift_plain_metrics.csv).  Both
command-line drivers run a build."""
import os
import random
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import shift_ref as SR
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu

BASE18 = ["Step", "Time", "AspectRatio", "EquiaxedFraction", "NucleationDensity", "DefectDensity", "AvgGrainSize", "GrainCount",
          "W_Count", "Re_Count", "C_Count", "NucleationCount", "G_over_R", "G_phys", "R_phys", "G_over_R_phys", "CET_Class",
          "CET_Detected"]
PATH_LASER = dict(power=60.0, path=dict(pattern="serpentine", speed=4.0, hatch=5.0), depth=2)


def _run(prefix, L, **kw):
    import kmc_simulation
    base = dict(L=L, n_steps=40, temp=3000.0, defect_fraction=0.02, n_seeds=6, impurity_c=0.1, output_prefix=prefix, metrics_every=20,
                build=dict(layers=3, thickness=4, T=2900.0))
    base.update(kw)
    out = kmc_simulation.run_kmc(**base)
    ends = (random.random(), float(np.random.random()))
    return out, open(f"outputs/{prefix}/metrics.csv", "rb").read(), ends, dict(kmc_simulation.last_run_info)


def _same_run(a, b):
    (fa, ma, ea, ia), (fb, mb, eb, ib) = a, b
    assert ma == mb and ea == eb and ia == ib
    for x, y in zip(fa, fb):
        assert np.array_equal(np.asarray(x).view(np.int64) if np.asarray(x).dtype == np.float64 else x,
                              np.asarray(y).view(np.int64) if np.asarray(y).dtype == np.float64 else y)


@pytest.mark.parametrize("L,laser", [(16, None), (24, PATH_LASER)])
def test_repeatable_and_equal_to_the_host_route(L, laser, tmp_path, monkeypatch):
    import cetkmc
    monkeypatch.chdir(tmp_path)
    kw = dict(layer_metrics=True, **(dict(laser=laser, thermal_scheme="implicit") if laser else {}))
    a = _run("a", L, **kw)
    b = _run("b", L, **kw)
    _same_run(a, b)
    info = a[3]["build"]
    assert (info["layers"], info["thickness"], info["retired_planes"], info["complete"]) == (3, 4, 8, True) and sum(info["dropped"]) == 2 * 4 * L * L
    assert (a[3]["beam"]["table_uploads"] == 3) if laser else ("beam" not in a[3])

    calls = []

    def by_host(self, d, fill_state=0, fill_T=None, T_mode="value", fill_theta=0.0, fill_phi=0.0):
        out, info = SR.shift_fields(self.download(defects=True), d, fill_state=fill_state, fill_T=fill_T, T_mode=T_mode,
                                    fill_theta=fill_theta, fill_phi=fill_phi)
        self.upload(out["state"], out["theta"], out["phi"], out["T"], out["defects"])
        calls.append(tuple(d))
        return dict(info, calls=len(calls))
    monkeypatch.setattr(cetkmc.Engine, "shift", by_host)
    c = _run("c", L, **kw)
    assert calls == [(-4, 0, 0)] * 2
    _same_run(a, c)


def test_build_layers_csv(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    L, h, N = 16, 4, 3
    seen = []
    real = kmc_simulation._add_layer_columns

    def spy(row, profile, L_):
        planes = real(row, profile, L_)
        seen.append((int(row["Step"]), planes))
        return planes
    monkeypatch.setattr(kmc_simulation, "_add_layer_columns", spy)
    _run("csv", L, layer_metrics=True, solid_metrics=True, origin_metrics=True)
    df = pd.read_csv("outputs/csv/build_layers.csv")
    assert len(df) == L + (N - 1) * h and df["BuildHeight"].tolist() == list(range(L + (N - 1) * h))
    assert df["Layer"].tolist() == [0] * h + [1] * h + [2] * L and df["Plane"].tolist() == list(range(h)) * 2 + list(range(L))
    assert {"layer_n_occ", "solid_n_rec", "origin_n_occ", "origin_ev_dep"} <= set(df.columns)
    tables = dict(seen)                                     # step -> the per-plane table of that metrics row
    assert sorted(tables) == [0, 20, 39, 40, 60, 79, 80, 100, 119]
    for layer, first, count in ((0, 0, h), (1, h, h), (2, 2 * h, L)):
        t = tables[40 * (layer + 1) - 1]
        rows = df.iloc[first:first + count]
        for col, values in t.items():
            if col != "plane":
                assert np.array_equal(rows[f"layer_{col}"].to_numpy(), np.asarray(values)[:count]), (layer, col)
    m = pd.read_csv("outputs/csv/metrics.csv")
    assert m["Layer"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and m["Step"].tolist() == sorted(tables) and list(m.columns)[-1] == "Layer"
    assert list(m.columns)[:18] == BASE18
    # the maps moved with the part: what the second layer's planes recorded is still there when they retire with the rest
    assert int(df["solid_n_rec"].sum()) > 0 and int(df["origin_n_dep"].sum() + df["origin_n_nuc"].sum() + df["origin_n_att"].sum()) > 0


def test_without_a_build_nothing_changes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _run("plain", 16, build=None, n_steps=47)
    # byte for byte the file the PARENT's run_kmc wrote at these arguments (recorded on an MI355X: tests/golden)
    assert open("outputs/plain/metrics.csv", "rb").read() == open(os.path.join(GOLDEN, "shift_plain_metrics.csv"), "rb").read()
    m = pd.read_csv("outputs/plain/metrics.csv")
    assert list(m.columns) == BASE18 and m["Step"].tolist() == [0, 20, 40, 46]
    assert not os.path.exists("outputs/plain/build_layers.csv")
    import kmc_simulation
    assert "build" not in kmc_simulation.last_run_info


@pytest.mark.parametrize("tool,args,metrics", [
    ("main.py", ["--levels", "0.1"], "outputs/impurity_c_10/metrics.csv"),
    ("gv_sweep.py", ["--temps", "3000", "--nu-dep", "2e13"], "outputs/gv_sweep/T3000_V2e+13_c_20/metrics.csv"),
])
def test_command_line(tool, args, metrics, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(PKG, tool), "--L", "16", "--steps", "20", *args, "--layers", "--build-layers", "2",
                        "--layer-thickness", "5", "--layer-T", "2950"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = pd.read_csv(tmp_path / metrics)
    assert m["Layer"].tolist() == [0, 0, 1] and m["Step"].tolist() == [0, 19, 39]      # (rows: every 200 steps and at a layer's end)
    assert len(pd.read_csv((tmp_path / metrics).parent / "build_layers.csv")) == 16 + 5
    r = subprocess.run([sys.executable, os.path.join(PKG, tool), "--L", "16", "--steps", "20", *args, "--build-layers", "2"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--layer-thickness" in r.stderr
