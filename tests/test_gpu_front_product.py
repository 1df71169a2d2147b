"""The measured front columns in the product layer: run_kmc(front_metrics=True) in mode A, mode A with a laser and mode B,
run_kmc_ensemble(front_metrics=True) against the sequential runs, and the front columns of gv_sweep's map."""
import csv

import numpy as np
import pandas as pd
import pytest

from front_ref import U, front_ref, front_ref_stats, sum_bound

pytestmark = pytest.mark.gpu

L, N_STEPS, EVERY = 12, 230, 50
LASER = dict(power=150.0, start=2.0, speed=0.5)
BASE18 = ["Step", "Time", "AspectRatio", "EquiaxedFraction", "NucleationDensity", "DefectDensity", "AvgGrainSize", "GrainCount",
          "W_Count", "Re_Count", "C_Count", "NucleationCount", "G_over_R", "G_phys", "R_phys", "G_over_R_phys", "CET_Class",
          "CET_Detected"]


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


@pytest.mark.parametrize("variant", ["A", "A_laser", "B"])
def test_run_kmc_front_columns(variant, tmp_path, monkeypatch):
    import cetkmc
    import kmc_simulation
    import metrics
    from constants import T_MELT, VOXEL_SIZE
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, impurity_c=0.1, defect_fraction=0.01, metrics_every=EVERY)
    kw.update({"A": {}, "A_laser": dict(laser=LASER), "B": dict(mode="B", box=L)}[variant])
    kmc_simulation.run_kmc(output_prefix="plain_0", **kw)
    # the lattice of every row, downloaded where the row is formed
    seen = []
    orig = cetkmc.Engine.front_stats

    def spy(self, inv_dx=None):
        d = self.download()
        seen.append((d["state"], d["T"]))
        return orig(self, inv_dx)
    monkeypatch.setattr(cetkmc.Engine, "front_stats", spy)
    kmc_simulation.run_kmc(output_prefix="front_0", front_metrics=True, **kw)
    monkeypatch.setattr(cetkmc.Engine, "front_stats", orig)

    plain, front = _rows("outputs/plain_0/metrics.csv"), _rows("outputs/front_0/metrics.csv")
    assert plain[0] == BASE18 and front[0] == BASE18 + list(metrics.FRONT_COLUMNS) + ["V_front"]
    assert len(plain) == len(front) >= 5 and [r[:18] for r in front] == plain           # the 18 columns: the same text
    df = pd.read_csv("outputs/front_0/metrics.csv", float_precision="round_trip")
    assert len(seen) == len(df)
    prev = None
    for q, (state, T) in enumerate(seen):
        row = df.iloc[q].to_dict()
        s = front_ref_stats(front_ref(state, T, float(T_MELT), 1.0 / VOXEL_SIZE), T)
        want = metrics.front_metrics(s, L, VOXEL_SIZE)
        n = s["n_front"]
        assert n > 0
        for k in ("FrontVoxels", "MeltVoxels", "MeltDepth", "MeltLength", "MeltWidth"):
            assert int(row[k]) == want[k], (q, k)
        assert row["Front_i"] == want["Front_i"]
        assert row["G_front_max"] == want["G_front_max"]
        for k, a, ulp in (("G_front", "abs_G", True), ("Gi_front", "abs_gi", False), ("T_front", "abs_T", False)):
            bound = sum_bound(n, s[a], ulp) / n + 2 * U * abs(want[k])                  # the sum's bound + the division
            assert abs(row[k] - want[k]) <= bound, (q, k, row[k], want[k], bound)
        assert abs(row["Undercooling_front"] - want["Undercooling_front"]) <= sum_bound(n, s["abs_T"]) / n + 4 * U * float(T_MELT)
        assert row["V_front"] == metrics.front_velocity(row, prev, VOXEL_SIZE), q
        prev = row
    assert df["V_front"].iloc[0] == 0.0
    print(f"{variant}: G_front {df['G_front'].tolist()} Front_i {df['Front_i'].tolist()} V_front {df['V_front'].tolist()} "
          f"MeltVoxels {df['MeltVoxels'].tolist()}")


def test_ensemble_rows_equal_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    cfgs = [dict(impurity_c=0.05 * (r + 1), seed=42 + r, defect_fraction=0.01 * r, temp=2800 + 150 * r, output_prefix=f"e{r}_{r}")
            for r in range(3)]
    kmc_simulation.run_kmc_ensemble(cfgs, L, N_STEPS, rng="reference", metrics_every=EVERY, front_metrics=True)
    for c in cfgs:
        kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, metrics_every=EVERY, front_metrics=True,
                               **dict(c, output_prefix="seq_" + c["output_prefix"]))
        a, b = (f"outputs/{p}{c['output_prefix']}/metrics.csv" for p in ("", "seq_"))
        assert open(a, "rb").read() == open(b, "rb").read(), c
        assert "V_front" in pd.read_csv(a).columns
    # without the option the ensemble's files have the 18 columns
    kmc_simulation.run_kmc_ensemble([dict(cfgs[0], output_prefix="p0_0")], L, 60, metrics_every=EVERY)
    assert _rows("outputs/p0_0/metrics.csv")[0] == BASE18


def test_gv_sweep_front_columns(tmp_path, monkeypatch):
    import gv_sweep
    monkeypatch.chdir(tmp_path)
    kw = dict(L=L, n_steps=N_STEPS, temps=(2800.0,), nu_deps=(2e13,), carbon=0.1)
    m = gv_sweep.gv_sweep(front=True, laser_powers=(60.0, 400.0), scan_speeds=(0.5,), laser_start=3.0, **kw)
    on_disk = pd.read_csv("outputs/gv_sweep/gv_map.csv")
    assert list(on_disk.columns) == list(m.columns) and len(m) == 2
    assert list(m.columns[-3:]) == ["G_front_K_per_m", "V_front_m_per_s", "G_over_V_front"]
    assert m["G_K_per_m"].iloc[0] == m["G_K_per_m"].iloc[1]                  # the nominal abscissa cannot tell the beams apart
    assert m["G_front_K_per_m"].iloc[0] != m["G_front_K_per_m"].iloc[1]      # the measured one does
    for q in range(2):
        g, v, gv = (m[c].iloc[q] for c in ("G_front_K_per_m", "V_front_m_per_s", "G_over_V_front"))
        assert g > 0 and gv == (g / v if v != 0.0 else np.inf)
    print(m[["power", "G_K_per_m", "G_front_K_per_m", "V_front_m_per_s", "G_over_V_front"]].to_string(index=False))
    m0 = gv_sweep.gv_sweep(**kw)
    assert list(pd.read_csv("outputs/gv_sweep/gv_map.csv").columns) == list(m0.columns) == [
        "T_sub", "nu_dep", "G_K_per_m", "V_m_per_s", "G_over_V", "AspectRatio", "EquiaxedFraction", "GrainCount",
        "NucleationCount", "CET_Class", "CET_Detected"]
    assert _rows("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv")[0] == BASE18
