"""The solidification map in the product layer: run_kmc(solid_metrics=True) in both modes, with a laser and beside the grain
columns; run_kmc_ensemble against the sequential runs; gv_sweep's --solid columns; the refusals.

The columns, solid_layers.csv and solid_grains.csv are compared with metrics.solid_metrics of the NumPy comparator
(solid_ref.py), which a spy on the Engine drives from downloads of state and T at the very splits where run_kmc updates the
map (downloads change nothing).  Without the option the files, the arrays and the generators' end states are those of a run
with it, less the new columns."""
import csv
import os
import random

import numpy as np
import pandas as pd
import pytest

import solid_ref as SR

pytestmark = pytest.mark.gpu

N_STEPS, EVERY = 250, 80
BASE18 = ["Step", "Time", "AspectRatio", "EquiaxedFraction", "NucleationDensity", "DefectDensity", "AvgGrainSize", "GrainCount",
          "W_Count", "Re_Count", "C_Count", "NucleationCount", "G_over_R", "G_phys", "R_phys", "G_over_R_phys", "CET_Class",
          "CET_Detected"]


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


class Spy:
    """the comparator beside every Engine the product creates: begin / update / profile mirrored from downloads"""

    def __init__(self, monkeypatch):
        import cetkmc
        import metrics
        spy, E = self, cetkmc.Engine
        self.rows, self.updates, self.ref, self.remelted = [], [], None, 0
        begin, update, profile = E.solid_begin, E.solid_update, E.solid_profile

        def solid_begin(e):
            d = e.download()
            spy.ref = SR.SolidRef(d["state"], d["T"])
            begin(e)

        def solid_update(e, stamp, dt, inv_dx=None):
            d = e.download()
            info = update(e, stamp, dt, inv_dx)
            want = spy.ref.update(d["state"], d["T"], stamp, cetkmc.engine._default_inv_dx(), dt)
            assert info == want, (stamp, info, want)
            spy.remelted += want["n_cleared"]
            spy.updates.append((stamp, dt, want))
            return info

        def solid_profile(e, scales=None, grains=False, threshold=0.5, recluster=True):
            got = profile(e, scales, grains, threshold, recluster)
            assert spy.ref.ties(scales) == 0
            cl = e.clusters(0.5, labels=True)
            want = spy.ref.profile(scales, cl["labels"] if grains else None)
            SR.check_identities(spy.ref, want, scales, cl["labels"] if grains else None)
            assert SR.same_records(got["layers"], want["layers"]) == []
            assert not grains or SR.same_records(got["grains"], want["grains"]) == []
            spy.rows.append(metrics.solid_metrics(want, scales, spy.remelted, 0, cl))
            return got

        monkeypatch.setattr(E, "solid_begin", solid_begin)
        monkeypatch.setattr(E, "solid_update", solid_update)
        monkeypatch.setattr(E, "solid_profile", solid_profile)


def _run(prefix, **kw):
    import kmc_simulation
    out = kmc_simulation.run_kmc(output_prefix=prefix, **kw)
    return out, random.getstate(), np.random.get_state()


@pytest.mark.parametrize("variant", ["A_grains", "A_laser", "B", "B_supersteps"])
def test_run_kmc_solid_columns(variant, tmp_path, monkeypatch):
    import metrics
    monkeypatch.chdir(tmp_path)
    L = 16 if variant.startswith("B") else 12
    kw = dict(L=L, n_steps=N_STEPS, impurity_c=0.1, defect_fraction=0.01, metrics_every=EVERY)
    kw.update({"A_grains": dict(grain_metrics=True), "A_laser": dict(laser=dict(power=200.0, start=3.0, speed=0.5)),
               "B": dict(mode="B", box=8), "B_supersteps": dict(mode="B", box=L, thermal_cadence="supersteps")}[variant])
    (out0, py0, np0) = _run("plain_0", **kw)
    spy = Spy(monkeypatch)
    (out1, py1, np1) = _run("so_0", solid_metrics=True, solid_every=40 if variant == "A_laser" else 20, **kw)
    # the run itself is untouched: arrays, total time, both generators
    for a, b in zip(out0, out1):
        assert np.array_equal(a, b)
    assert py0 == py1 and all(np.array_equal(a, b) for a, b in zip(np0, np1))
    plain, so = _rows("outputs/plain_0/metrics.csv"), _rows("outputs/so_0/metrics.csv")
    mid = list(metrics.GRAIN_COLUMNS) if variant == "A_grains" else []
    assert plain[0] == BASE18 + mid and so[0] == BASE18 + mid + list(metrics.SOLID_COLUMNS)
    n0 = len(plain[0])
    assert len(plain) == len(so) >= 4 and [r[:n0] for r in so] == plain
    extra = {"solid_layers.csv"} | ({"solid_grains.csv"} if variant == "A_grains" else set())
    assert sorted(os.listdir("outputs/plain_0")) == [f for f in sorted(os.listdir("outputs/so_0")) if f not in extra]
    assert all(os.path.exists(f"outputs/so_0/{f}") for f in extra)
    # the splits: every multiple of solid_every up to the end, dt = temperature updates between them * 1e-6
    every = 40 if variant == "A_laser" else 20
    stamps = [u[0] for u in spy.updates]
    if variant == "B":
        assert all(b // every > a // every for a, b in zip([0] + stamps, stamps)) and len(stamps) >= 4
    else:
        assert stamps == list(range(every, N_STEPS + 1, every))
        assert all(u[1] == (every // 20) * 1e-6 for u in spy.updates)
    # columns and tables of every row against the comparator's
    df = pd.read_csv("outputs/so_0/metrics.csv", float_precision="round_trip")
    assert len(df) == len(spy.rows)
    for q, want in enumerate(spy.rows):
        for k in metrics.SOLID_COLUMNS:
            assert df[k].iloc[q] == want[k], (q, k, df[k].iloc[q], want[k])
    lay = pd.read_csv("outputs/so_0/solid_layers.csv", float_precision="round_trip")
    assert len(lay) == L * len(spy.rows) and list(lay.columns) == list(spy.rows[0]["planes"])
    assert lay["Step"].tolist() == [s for s in df["Step"].tolist() for _ in range(L)]
    for k in lay.columns[1:]:
        assert np.array_equal(lay[k].to_numpy(), np.concatenate([w["planes"][k] for w in spy.rows])), k
    if variant == "A_grains":
        g = pd.read_csv("outputs/so_0/solid_grains.csv", float_precision="round_trip")
        want = spy.rows[-1]["grains"]
        assert len(g) == int(df["GrainCount"].iloc[-1]) and list(g.columns) == list(want) and "aspect" in want
        for k, v in want.items():
            assert np.array_equal(g[k].to_numpy(), v), k
    last = df.iloc[-1]
    print(f"{variant}: updates {len(stamps)} SolidVoxels {df['SolidVoxels'].tolist()} Remelted {df['Remelted'].tolist()} "
          f"G {last['G_solid']:.3e} Gi {last['Gi_solid']:.3e} cool {last['Cool_solid']:.3e} V {last['V_solid']:.3e}")
    assert df["SolidVoxels"].iloc[-1] >= 100 and (df["SolidVoxels"].diff().dropna() >= 0).any()
    assert last["G_solid"] > 0 and last["T_solid"] > 0
    assert last["V_solid"] == (-last["Cool_solid"] / last["Gi_solid"] if last["Gi_solid"] != 0 else 0.0)


def test_ensemble_rows_equal_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    import metrics
    monkeypatch.chdir(tmp_path)
    L = 12
    cfgs = [dict(impurity_c=0.05 * (r + 1), seed=42 + r, defect_fraction=0.01 * r, temp=2800 + 150 * r, output_prefix=f"e{r}_{r}")
            for r in range(3)]
    kw = dict(metrics_every=EVERY, solid_metrics=True, grain_metrics=True)
    out = kmc_simulation.run_kmc_ensemble(cfgs, L, N_STEPS, rng="reference", **kw)
    for r, c in enumerate(cfgs):
        seq = kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, **kw, **dict(c, output_prefix="seq_" + c["output_prefix"]))
        for f in ("metrics.csv", "grains.csv", "solid_layers.csv", "solid_grains.csv"):
            a, b = (f"outputs/{p}{c['output_prefix']}/{f}" for p in ("", "seq_"))
            assert open(a, "rb").read() == open(b, "rb").read(), (c, f)
        assert all(np.array_equal(a, b) for a, b in zip(out[r], seq))
    # the counter ensemble against mode B, box = L, super-step cadence
    c = dict(cfgs[1], output_prefix="c1_1")
    kmc_simulation.run_kmc_ensemble([c], L, N_STEPS, rng="counter", metrics_every=EVERY, solid_metrics=True)
    kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, mode="B", box=L, thermal_cadence="supersteps", metrics_every=EVERY, solid_metrics=True,
                           **dict(c, output_prefix="seq_c1_1"))
    for f in ("metrics.csv", "solid_layers.csv"):
        assert open(f"outputs/c1_1/{f}", "rb").read() == open(f"outputs/seq_c1_1/{f}", "rb").read(), f
    # without the option: no solid file, the columns of before
    kmc_simulation.run_kmc_ensemble([dict(cfgs[0], output_prefix="p0_0")], L, N_STEPS, metrics_every=EVERY)
    assert _rows("outputs/p0_0/metrics.csv")[0] == BASE18 and not os.path.exists("outputs/p0_0/solid_layers.csv")
    assert [r[:18] for r in _rows("outputs/seq_e0_0/metrics.csv")] == _rows("outputs/p0_0/metrics.csv")
    assert _rows("outputs/seq_e0_0/metrics.csv")[0][-len(metrics.SOLID_COLUMNS):] == list(metrics.SOLID_COLUMNS)


def test_gv_sweep_solid_columns(tmp_path, monkeypatch):
    import gv_sweep
    monkeypatch.chdir(tmp_path)
    kw = dict(L=12, n_steps=N_STEPS, temps=(2800.0,), nu_deps=(2e13, 2e14), carbon=0.1)          # a 2 x 1 map
    m = gv_sweep.gv_sweep(solid=True, **kw)
    on_disk = pd.read_csv("outputs/gv_sweep/gv_map.csv", float_precision="round_trip")
    assert list(on_disk.columns) == list(m.columns) and len(m) == 2
    assert list(m.columns[-3:]) == ["G_solid_K_per_m", "V_solid_m_per_s", "G_over_V_solid"]
    for q, v in enumerate(("2e+13", "2e+14")):
        last = pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/metrics.csv").iloc[-1]          # parsed as gv_sweep parses it
        assert m["G_solid_K_per_m"].iloc[q] == last["G_solid"] and m["V_solid_m_per_s"].iloc[q] == last["V_solid"]
        assert m["G_over_V_solid"].iloc[q] == (last["G_solid"] / last["V_solid"] if last["V_solid"] != 0 else float("inf"))
        assert os.path.exists(f"outputs/gv_sweep/T2800_V{v}_c_10/solid_layers.csv")
    m0 = gv_sweep.gv_sweep(**kw)
    assert list(m0.columns) == ["T_sub", "nu_dep", "G_K_per_m", "V_m_per_s", "G_over_V", "AspectRatio", "EquiaxedFraction",
                                "GrainCount", "NucleationCount", "CET_Class", "CET_Detected"]
    assert m0.equals(m[list(m0.columns)])
    assert _rows("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv")[0] == BASE18


def test_refusals(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(L=12, n_steps=40, solid_metrics=True)
    for every in (30, 0, -20, 10, 20.0):
        with pytest.raises(ValueError, match="multiple of 20"):
            kmc_simulation.run_kmc(solid_every=every, **kw)
        with pytest.raises(ValueError, match="multiple of 20"):
            kmc_simulation.run_kmc_ensemble([dict(output_prefix="x_0")], 12, 40, solid_metrics=True, solid_every=every)
    with pytest.raises(ValueError, match="checkpoint"):
        kmc_simulation.run_kmc(checkpoint_every=20, **kw)
    with pytest.raises(ValueError, match="checkpoint"):
        kmc_simulation.run_kmc(resume_from="nowhere.npz", **kw)
    assert not os.path.exists("outputs")                       # refused before anything was created
    kmc_simulation.run_kmc(L=12, n_steps=40, solid_every=30, output_prefix="ok_0")      # without the option the value is not looked at
    assert _rows("outputs/ok_0/metrics.csv")[0] == BASE18
