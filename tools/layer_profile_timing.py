"""Layer profile of a replica ensemble: Ensemble.layer_profile on the last analysis (one streaming pass on the device,
R x L x 144 bytes to the host) against the route it replaces -- download the labels and the state of every replica and
count with NumPy (tests/layer_ref.py).  Prints one JSON line per (L, R) and, with --out, writes the list to a file
(profiles/layer_profile.json).

    python tools/layer_profile_timing.py [--config 30,64 --config 128,16] [--reps 20] [--out profiles/layer_profile.json]

``call_ms`` is the host time of one Ensemble.layer_profile(recluster=False) call (table upload, three launches, copy,
synchronisation; median of --reps calls after a warm-up): an upper bound of the kernels' device time.  ``alg_bytes`` are the
algorithmic bytes of the pass (5 B per voxel: label i32 + state u8), ``alg_GBps_call`` those bytes over the whole call -- a
lower bound of the stream rate.  ``download_route_ms`` = the analysis with the label download, the state download of every
replica and the NumPy count; the clustering itself is needed by both routes (``analyze_first_call_ms`` is the first
Ensemble.analyze of the handle without labels, allocations included)."""
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
import layer_ref as LR  # noqa: E402


def one(L, R, reps):
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1 * (r % 3)) for r in range(R)])
    T, zi = np.full((L, L, L), float(constants.T_SUB)), np.zeros((L, L, L), np.int64)
    for r in range(R):
        state, theta, phi = LR.random_blocks(L, L * 1000 + r)
        ens.replica(r).upload(state, theta, phi, T, zi)
    t0 = time.perf_counter()
    ens.analyze(0.5, labels=False)
    t_an = time.perf_counter() - t0
    ens.layer_profile(recluster=False)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = ens.layer_profile(recluster=False)
        t.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    an = ens.analyze(0.5, labels=True)
    states = [ens.replica(r).download(theta=False, phi=False, T=False)["state"] for r in range(R)]
    t_down = time.perf_counter() - t0
    t0 = time.perf_counter()
    ar = float(constants.CET_AR_THRESHOLD)
    want = [LR.layer_ref(a["clusters"]["labels"], s, a["clusters"]["bbox"], a["clusters"]["first"], ar) for a, s in zip(an, states)]
    t_ref = time.perf_counter() - t0
    assert all(LR.same({k: got[k][r] for k in LR.FIELDS}, want[r]) == [] for r in range(R))
    ens.close()
    return dict(L=L, R=R, reps=reps, call_ms=1e3 * float(np.median(t)), call_ms_min=1e3 * min(t), analyze_first_call_ms=1e3 * t_an,
                download_route_ms=1e3 * (t_down + t_ref), analyze_and_download_ms=1e3 * t_down, numpy_count_ms=1e3 * t_ref,
                d2h_bytes=R * L * 144, download_route_bytes=R * L ** 3 * 5, alg_bytes=5 * R * L ** 3)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", help="L,R (repeatable; default 30,64 and 128,16)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the records to this JSON list")
    a = ap.parse_args()
    out = []
    for c in a.config or ["30,64", "128,16"]:
        L, R = (int(x) for x in c.split(","))
        rec = one(L, R, a.reps)
        rec["alg_GBps_call"] = rec["alg_bytes"] / (rec["call_ms"] * 1e-3) / 1e9
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        json.dump(old + out, open(a.out, "w"), indent=1)
