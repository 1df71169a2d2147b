"""Texture profile of a replica ensemble: Ensemble.texture_profile on the last analysis (one streaming pass on the device,
R x L x (4 n_bins + 4) x 8 bytes to the host) against the route it replaces -- download the labels, theta and phi of every
replica and bin with NumPy (tests/texture_ref.py).  Prints one JSON line per (L, R) and, with --out, writes the list to a
file (profiles/texture_profile.json).

    python tools/texture_profile_timing.py [--config 30,64 --config 128,16] [--bins 36] [--reps 20] [--out profiles/texture_profile.json]

``call_ms`` is the host time of one Ensemble.texture_profile(recluster=False) call, which ends in a stream synchronisation
(result allocation, memset, one launch, copy, split on the host; median of --reps calls after a warm-up): an upper bound of
the kernel's device time -- the kernel alone is read from a separate run of this tool under rocprofv3 --kernel-trace --stats
(k_texture_profile).  ``alg_bytes`` are the algorithmic bytes of the pass (28 B per voxel: label i32 + three doubles),
``alg_GBps_call`` those bytes over the whole call -- a lower bound of the stream rate.  ``download_route_ms`` = the analysis
with the label download, the theta / phi download of every replica and the NumPy binning; the clustering itself is needed by
both routes.  The two results are compared (==) before anything is reported."""
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
import texture_ref as TR  # noqa: E402


def one(L, R, nb, reps):
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1 * (r % 3)) for r in range(R)])
    T, zi = np.full((L, L, L), float(constants.T_SUB)), np.zeros((L, L, L), np.int64)
    for r in range(R):
        state, theta, phi = LR.random_blocks(L, L * 1000 + r)
        ens.replica(r).upload(state, theta, phi, T, zi)
    ens.analyze(0.5, labels=False)
    ens.texture_profile(n_bins=nb, recluster=False)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = ens.texture_profile(n_bins=nb, recluster=False)
        t.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    an = ens.analyze(0.5, labels=True)
    ang = [ens.replica(r).download(state=False, T=False) for r in range(R)]
    t_down = time.perf_counter() - t0
    t0 = time.perf_counter()
    ge, pe = TR.edges_cos(nb, 180.0), TR.edges_cos(nb, 90.0)
    want = [TR.texture_ref(a["clusters"]["labels"], d["theta"], d["phi"], ge, pe) for a, d in zip(an, ang)]
    t_ref = time.perf_counter() - t0
    near = sum(TR.n_ambiguous((TR.face_values(a["clusters"]["labels"], d["theta"], d["phi"]),
                               TR.pole_values(a["clusters"]["labels"], d["theta"], d["phi"], (1.0, 0.0, 0.0))), ge, pe)
               for a, d in zip(an, ang))
    differ = sum(len(TR.same({k: got[k][r] for k in TR.FIELDS}, want[r])) for r in range(R))
    assert differ == 0 or near > 0, (differ, near)
    ens.close()
    return dict(L=L, R=R, n_bins=nb, reps=reps, call_ms=1e3 * float(np.median(t)), call_ms_min=1e3 * min(t),
                download_route_ms=1e3 * (t_down + t_ref), analyze_and_download_ms=1e3 * t_down, numpy_binning_ms=1e3 * t_ref,
                d2h_bytes=R * L * (4 * nb + 4) * 8, download_route_bytes=R * L ** 3 * 20, alg_bytes=28 * R * L ** 3,
                grain_faces=int(got["gb_hist"].sum()), near_edge_values=near, planes_differing=differ)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", action="append", help="L,R (repeatable; default 30,64 and 128,16)")
    ap.add_argument("--bins", type=int, default=36)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None, help="append the records to this JSON list")
    a = ap.parse_args()
    out = []
    for c in a.config or ["30,64", "128,16"]:
        L, R = (int(x) for x in c.split(","))
        rec = one(L, R, a.bins, a.reps)
        rec["alg_GBps_call"] = rec["alg_bytes"] / (rec["call_ms"] * 1e-3) / 1e9
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        json.dump(old + out, open(a.out, "w"), indent=1)
