"""The origin map in the product layer: run_kmc(origin_metrics=True) in both modes, with a laser and beside the grain columns;
run_kmc_ensemble against the sequential runs; main.py --origin and gv_sweep's --origin columns; the refusals.

The columns, origin_layers.csv and origin_grains.csv are compared with metrics.origin_metrics of the comparator
(origin_ref.py), which a spy on the Engine builds from the event logs of the very stepping calls the driver makes (Mode B: it
asks those calls for their events, which changes nothing else).  Without the option the files, the arrays and the generators'
end states are those of a run with it, less the new columns."""
import csv
import os
import random
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest

import origin_ref as OR
from conftest import PKG

pytestmark = pytest.mark.gpu

N_STEPS, EVERY = 400, 150
BASE18 = ["Step", "Time", "AspectRatio", "EquiaxedFraction", "NucleationDensity", "DefectDensity", "AvgGrainSize", "GrainCount",
          "W_Count", "Re_Count", "C_Count", "NucleationCount", "G_over_R", "G_phys", "R_phys", "G_over_R_phys", "CET_Class",
          "CET_Detected"]
FIELDS = tuple(f for f in OR.REC_FIELDS if f != "pad")


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.reader(f))


class Spy:
    """the comparator beside every Engine the product creates: begin, the stepping calls and the profile mirrored"""

    def __init__(self, monkeypatch):
        import cetkmc
        import metrics
        spy, E = self, cetkmc.Engine
        self.rows, self.calls = [], 0
        begin, steps, supers, profile = E.origin_begin, E.run_steps, E.run_supersteps, E.origin_profile

        def origin_begin(e):
            L = e.L
            spy.words, spy.census, spy.seq = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64), 0
            begin(e)

        def run_steps(e, *a, **kw):
            r = steps(e, *a, **kw)
            spy.seq = OR.absorb(spy.words, spy.census, r["events"][:r["done"]], spy.seq, 1, e.L)
            spy.calls += 1
            return r

        def run_supersteps(e, *a, **kw):
            r = supers(e, *a, **dict(kw, want_events=True))
            spy.seq = OR.absorb(spy.words, spy.census, r["events"], spy.seq, r["domains"], e.L)
            spy.calls += 1
            return r

        def origin_profile(e, grains=False, threshold=0.5, recluster=True):
            got = profile(e, grains, threshold, recluster)
            assert np.array_equal(e.origin_words(), spy.words) and e.origin_seq() == spy.seq
            census = e.origin_census()
            assert np.array_equal(census, spy.census)
            cl = e.clusters(0.5, labels=True)
            lay, gr = OR.profile(spy.words, e.download()["state"], cl["labels"] if grains else None, len(cl["size"]))
            assert [f for f in FIELDS if not np.array_equal(got["layers"][f], lay[f])] == []
            assert not grains or [f for f in FIELDS if not np.array_equal(got["grains"][f], gr[f])] == []
            want = dict(layers={f: lay[f] for f in FIELDS}, grains=None if gr is None else {f: gr[f] for f in FIELDS})
            spy.rows.append(metrics.origin_metrics(want, spy.census.copy(), 0))
            return got

        monkeypatch.setattr(E, "origin_begin", origin_begin)
        monkeypatch.setattr(E, "run_steps", run_steps)
        monkeypatch.setattr(E, "run_supersteps", run_supersteps)
        monkeypatch.setattr(E, "origin_profile", origin_profile)


def _run(prefix, **kw):
    import kmc_simulation
    out = kmc_simulation.run_kmc(output_prefix=prefix, **kw)
    return out, random.getstate(), np.random.get_state()


@pytest.mark.parametrize("variant", ["A_grains", "A_laser", "B", "B_single"])
def test_run_kmc_origin_columns(variant, tmp_path, monkeypatch):
    import metrics
    monkeypatch.chdir(tmp_path)
    L = 16 if variant == "B" else 12
    kw = dict(L=L, n_steps=N_STEPS, impurity_c=0.1, defect_fraction=0.01, metrics_every=EVERY)
    kw.update({"A_grains": dict(grain_metrics=True), "A_laser": dict(laser=dict(power=200.0, start=3.0, speed=0.5)),
               "B": dict(mode="B", box=8), "B_single": dict(mode="B", box=L, thermal_cadence="supersteps")}[variant])
    (out0, py0, np0) = _run("plain_0", **kw)
    spy = Spy(monkeypatch)
    (out1, py1, np1) = _run("or_0", origin_metrics=True, **kw)
    # the run itself is untouched: arrays, total time, both generators
    for a, b in zip(out0, out1):
        assert np.array_equal(a, b)
    assert py0 == py1 and all(np.array_equal(a, b) for a, b in zip(np0, np1))
    plain, orr = _rows("outputs/plain_0/metrics.csv"), _rows("outputs/or_0/metrics.csv")
    mid = list(metrics.GRAIN_COLUMNS) if variant == "A_grains" else []
    assert plain[0] == BASE18 + mid and orr[0] == BASE18 + mid + list(metrics.ORIGIN_COLUMNS)
    n0 = len(plain[0])
    assert len(plain) == len(orr) >= 4 and [r[:n0] for r in orr] == plain
    extra = {"origin_layers.csv"} | ({"origin_grains.csv"} if variant == "A_grains" else set())
    assert sorted(os.listdir("outputs/plain_0")) == [f for f in sorted(os.listdir("outputs/or_0")) if f not in extra]
    assert all(os.path.exists(f"outputs/or_0/{f}") for f in extra)
    # columns and tables of every row against the comparator's
    df = pd.read_csv("outputs/or_0/metrics.csv", float_precision="round_trip")
    assert len(df) == len(spy.rows) and spy.calls >= 3
    for q, want in enumerate(spy.rows):
        for k in metrics.ORIGIN_COLUMNS:
            assert df[k].iloc[q] == want[k], (q, k, df[k].iloc[q], want[k])
    lay = pd.read_csv("outputs/or_0/origin_layers.csv", float_precision="round_trip")
    assert len(lay) == L * len(spy.rows) and list(lay.columns) == list(spy.rows[0]["planes"])
    assert lay["Step"].tolist() == [s for s in df["Step"].tolist() for _ in range(L)]
    for k in lay.columns[1:]:
        assert np.array_equal(lay[k].to_numpy(), np.concatenate([w["planes"][k] for w in spy.rows])), k
    if variant == "A_grains":
        g = pd.read_csv("outputs/or_0/origin_grains.csv", float_precision="round_trip")
        want = spy.rows[-1]["grains"]
        assert len(g) == int(df["GrainCount"].iloc[-1]) and list(g.columns) == list(want)
        for k, v in want.items():
            assert np.array_equal(g[k].to_numpy(), v), k
    last = df.iloc[-1]
    print(f"{variant}: calls {spy.calls} seq {spy.seq} " + " ".join(f"{k}={last[k]}" for k in metrics.ORIGIN_COLUMNS))
    filled = sum(int(last[k]) for k in ("Origin_dep", "Origin_nuc", "Origin_att", "Origin_hop"))
    assert filled >= 100 and last["Nuc_events"] >= last["Origin_nuc"] > 0 and last["Origin_unrecorded"] > 0
    assert last["Nuc_events"] <= last["NucleationCount"]
    assert last["Grains_born_nuc"] + last["Grains_born_dep"] + last["Grains_born_att"] + last["Grains_born_hop"] + \
        last["Grains_substrate"] == last["GrainCount"]
    assert 0.0 < last["Nucleated_voxel_frac"] <= 1.0 and 0.0 <= last["Nucleated_grain_volume_frac"] <= 1.0


def test_ensemble_rows_equal_sequential(tmp_path, monkeypatch):
    import kmc_simulation
    import metrics
    monkeypatch.chdir(tmp_path)
    L = 12
    cfgs = [dict(impurity_c=0.05 * (r + 1), seed=42 + r, defect_fraction=0.01 * r, temp=2800 + 150 * r, output_prefix=f"e{r}_{r}")
            for r in range(3)]
    kw = dict(metrics_every=EVERY, origin_metrics=True, grain_metrics=True)
    out = kmc_simulation.run_kmc_ensemble(cfgs, L, N_STEPS, rng="reference", **kw)
    for r, c in enumerate(cfgs):
        seq = kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, **kw, **dict(c, output_prefix="seq_" + c["output_prefix"]))
        for f in ("metrics.csv", "grains.csv", "origin_layers.csv", "origin_grains.csv"):
            a, b = (f"outputs/{p}{c['output_prefix']}/{f}" for p in ("", "seq_"))
            assert open(a, "rb").read() == open(b, "rb").read(), (c, f)
        assert all(np.array_equal(a, b) for a, b in zip(out[r], seq))
    # the counter ensemble against mode B, box = L, super-step cadence
    c = dict(cfgs[1], output_prefix="c1_1")
    kmc_simulation.run_kmc_ensemble([c], L, N_STEPS, rng="counter", metrics_every=EVERY, origin_metrics=True)
    kmc_simulation.run_kmc(L=L, n_steps=N_STEPS, mode="B", box=L, thermal_cadence="supersteps", metrics_every=EVERY, origin_metrics=True,
                           **dict(c, output_prefix="seq_c1_1"))
    for f in ("metrics.csv", "origin_layers.csv"):
        assert open(f"outputs/c1_1/{f}", "rb").read() == open(f"outputs/seq_c1_1/{f}", "rb").read(), f
    assert not os.path.exists("outputs/c1_1/origin_grains.csv")
    # without the option: no origin file, the columns of before
    kmc_simulation.run_kmc_ensemble([dict(cfgs[0], output_prefix="p0_0")], L, N_STEPS, metrics_every=EVERY)
    assert _rows("outputs/p0_0/metrics.csv")[0] == BASE18 and not os.path.exists("outputs/p0_0/origin_layers.csv")
    assert [r[:18] for r in _rows("outputs/seq_e0_0/metrics.csv")] == _rows("outputs/p0_0/metrics.csv")
    assert _rows("outputs/seq_e0_0/metrics.csv")[0][-len(metrics.ORIGIN_COLUMNS):] == list(metrics.ORIGIN_COLUMNS)


def test_gv_sweep_and_main_origin(tmp_path, monkeypatch):
    import gv_sweep
    import metrics
    monkeypatch.chdir(tmp_path)
    kw = dict(L=12, n_steps=N_STEPS, temps=(2800.0,), nu_deps=(2e13, 2e14), carbon=0.1)          # a 2 x 1 map
    m = gv_sweep.gv_sweep(origin=True, **kw)
    on_disk = pd.read_csv("outputs/gv_sweep/gv_map.csv", float_precision="round_trip")
    assert list(on_disk.columns) == list(m.columns) and len(m) == 2
    assert list(m.columns[-2:]) == ["Nucleated_grain_volume_frac", "Nucleated_voxel_frac"]
    for q, v in enumerate(("2e+13", "2e+14")):
        last = pd.read_csv(f"outputs/gv_sweep/T2800_V{v}_c_10/metrics.csv").iloc[-1]          # parsed as gv_sweep parses it
        assert m["Nucleated_grain_volume_frac"].iloc[q] == last["Nucleated_grain_volume_frac"]
        assert m["Nucleated_voxel_frac"].iloc[q] == last["Nucleated_voxel_frac"] > 0
        assert os.path.exists(f"outputs/gv_sweep/T2800_V{v}_c_10/origin_layers.csv")
    m0 = gv_sweep.gv_sweep(**kw)
    assert list(m0.columns) == ["T_sub", "nu_dep", "G_K_per_m", "V_m_per_s", "G_over_V", "AspectRatio", "EquiaxedFraction",
                                "GrainCount", "NucleationCount", "CET_Class", "CET_Detected"]
    assert m0.equals(m[list(m0.columns)])
    assert _rows("outputs/gv_sweep/T2800_V2e+13_c_10/metrics.csv")[0] == BASE18
    # the command-line tool: one level, a short run
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "--L", "12", "--steps", "200", "--levels", "0.1", "--origin"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    head = _rows("outputs/impurity_c_10/metrics.csv")[0]
    assert head == BASE18 + list(metrics.ORIGIN_COLUMNS) and os.path.exists("outputs/impurity_c_10/origin_layers.csv")


def test_refusals(tmp_path, monkeypatch):
    import kmc_simulation
    monkeypatch.chdir(tmp_path)
    kw = dict(L=12, n_steps=40, origin_metrics=True)
    with pytest.raises(ValueError, match="checkpoint"):
        kmc_simulation.run_kmc(checkpoint_every=20, **kw)
    with pytest.raises(ValueError, match="checkpoint"):
        kmc_simulation.run_kmc(resume_from="nowhere.npz", **kw)
    assert not os.path.exists("outputs")                       # refused before anything was created
