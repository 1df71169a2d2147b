"""Per-grain table: Ensemble.grain_table / Engine.grain_table on the last clustering (memset, two launches, n x 160 bytes to
the host) against the route it replaces -- download the labels and the state and reduce with NumPy (tests/grain_ref.py).
Prints one JSON line per case and, with --out, writes the list to a file (profiles/grain_table.json).

    python tools/grain_table_timing.py [--reps 20] [--only NAME ...] [--out profiles/grain_table.json]

Cases: ensembles of continuous-orientation lattices at L = 30, R = 64 and L = 128, R = 16 (threshold 0.5), and a single
handle at L = 128 in the three regimes of the reduction by label: one grain (imported), the device clustering of continuous
orientations at thresholds 0.5 and 1.2, and singletons (imported; every occupied voxel its own grain).

``call_ms`` is the host time of one grain_table(recluster=False) call, which ends in a stream synchronisation (allocation,
memset, two launches, copy, split into arrays on the host; median of --reps calls after a warm-up): an upper bound of the
kernels' device time.  ``download_route_ms`` = the label and state downloads (5 B per voxel; the angles of the first voxels
are fetched outside the timed part) plus the NumPy reduction; the clustering itself is needed by both routes.  The two
results are compared (==, the angles as int64 views) before anything is reported, and the tool fails when the device call is
slower than the route it replaces."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cet-driven-simulation-for-3d-printing-am-kmc-approach_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cetkmc  # noqa: E402
import constants  # noqa: E402
import cluster_ref as CR  # noqa: E402
import grain_ref as GR  # noqa: E402
import layer_ref as LR  # noqa: E402


def _median_call(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = fn()
        t.append(time.perf_counter() - t0)
    return got, 1e3 * float(np.median(t)), 1e3 * min(t)


def _record(name, L, R, reps, call, n_grains, largest, t_down, t_ref):
    rec = dict(case=name, L=L, R=R, reps=reps, call_ms=call[0], call_ms_min=call[1], download_route_ms=1e3 * (t_down + t_ref),
               download_ms=1e3 * t_down, numpy_ms=1e3 * t_ref, grains=int(n_grains), largest_share=float(largest),
               d2h_bytes=int(n_grains) * GR.REC, download_route_bytes=5 * R * L ** 3, alg_bytes=5 * R * L ** 3)
    rec["speedup"] = rec["download_route_ms"] / rec["call_ms"]
    return rec


def ensemble(L, R, reps):
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1 * (r % 3)) for r in range(R)])
    T, zi = np.full((L, L, L), float(constants.T_SUB)), np.zeros((L, L, L), np.int64)
    for r in range(R):
        state, theta, phi = CR.continuous(L, 0.6, L * 1000 + r)
        ens.replica(r).upload(state, theta, phi, T, zi)
    ens.analyze(0.5, labels=False)
    got, ms, ms_min = _median_call(lambda: ens.grain_table(recluster=False), reps)
    ang = [ens.replica(r).download(state=False, T=False) for r in range(R)]
    t0 = time.perf_counter()
    lab = np.zeros((R, L, L, L), np.int32)
    ens._ck(ens.lib.cetkmc_ensemble_analysis_data(ens.h, None, None, None, lab.ctypes.data, None, None))
    st = [ens.replica(r).download(theta=False, phi=False, T=False)["state"] for r in range(R)]
    t_down = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = [GR.grain_ref(lab[r], st[r], ang[r]["theta"], ang[r]["phi"]) for r in range(R)]
    t_ref = time.perf_counter() - t0
    ens.close()
    assert all(GR.same(g, w) == [] for g, w in zip(got, want))
    n = np.concatenate([w["n"] for w in want])
    return _record(f"ensemble_L{L}_R{R}", L, R, reps, (ms, ms_min), len(n), max(w["n"].max() / w["n"].sum() for w in want), t_down, t_ref)


def single(name, L, reps):
    e = cetkmc.Engine(L)
    T, zi = np.full((L, L, L), float(constants.T_SUB)), np.zeros((L, L, L), np.int64)
    if name == "one_grain":
        raw, state = LR.one(L)
        theta, phi = GR.angles(L, 1)
        e.upload(state, theta, phi, T, zi)
        e.import_clusters(raw.astype(np.int32))
    elif name == "singletons":
        lab, state = GR.singletons(L)
        theta, phi = GR.angles(L, 2)
        e.upload(state, theta, phi, T, zi)
        e.import_clusters(lab)
    else:
        state, theta, phi = CR.continuous(L, 0.6, L)
        e.upload(state, theta, phi, T, zi)
        e.clusters(float(name.split("_")[1]))
    got, ms, ms_min = _median_call(lambda: e.grain_table(recluster=False), reps)
    ang = e.download(state=False, T=False)
    t0 = time.perf_counter()
    lab = np.zeros((L, L, L), np.int32)
    e._ck(e.lib.cetkmc_cluster_labels(e.h, lab.ctypes.data))
    st = e.download(theta=False, phi=False, T=False)["state"]
    t_down = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = GR.grain_ref(lab, st, ang["theta"], ang["phi"])
    t_ref = time.perf_counter() - t0
    e.close()
    assert GR.same(got, want) == []
    return _record(f"single_L{L}_{name}", L, 1, reps, (ms, ms_min), len(want["n"]), want["n"].max() / want["n"].sum(), t_down, t_ref)


CASES = {"ensemble_L30_R64": lambda reps: ensemble(30, 64, reps), "ensemble_L128_R16": lambda reps: ensemble(128, 16, reps),
         "single_L128_one_grain": lambda reps: single("one_grain", 128, reps),
         "single_L128_continuous_0.5": lambda reps: single("continuous_0.5", 128, reps),
         "single_L128_continuous_1.2": lambda reps: single("continuous_1.2", 128, reps),
         "single_L128_singletons": lambda reps: single("singletons", 128, reps)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", nargs="*", choices=sorted(CASES), help="a subset of the cases")
    ap.add_argument("--out", default=None, help="append the records to this JSON list")
    a = ap.parse_args()
    out = []
    for name in a.only or list(CASES):
        rec = CASES[name](a.reps)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        json.dump(old + out, open(a.out, "w"), indent=1)
    slower = [r["case"] for r in out if r["call_ms"] > r["download_route_ms"]]
    assert not slower, f"the device call is slower than the route it replaces in {slower}"
