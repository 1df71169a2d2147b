"""Origin map: the cost of absorbing a stepping call's event log, and origin_profile against the route it replaces -- download
state, labels and words and reduce them with NumPy (tests/origin_ref.py).  Prints one JSON line per case and, with --out,
appends the list to a file (profiles/origin_map.json).

    python tools/origin_map_timing.py [--reps 20] [--only NAME ...] [--out profiles/origin_map.json]

Cases.  ``absorb_L128``: a 200-step cetkmc_run_steps call (counter uniforms, no temperature update) on a handle with a map and
on one without, alternated: ``with_map_ms`` / ``without_map_ms`` are the medians of --reps host times of the call after a
warm-up, ``extra_ms`` their difference -- one launch of ceil(200 / 256) = 1 block behind the call's synchronisation, 64 B read
per record.  ``profile_*``: ensembles at L = 30, R = 64 and L = 128, R = 16, a single handle at L = 256: ``profile_ms`` is
one profile call with grain records (median of --reps after a warm-up, its copy to the host and synchronisation included),
``profile_route_ms`` the download of state, labels and words plus the NumPy profile; ``profile_bytes`` is what the kernel
moves by its algorithm, 13 B per voxel (8 B word, 4 B label, 1 B state).  ``e2e_L30`` / ``e2e_L128``: run_kmc with and without
origin_metrics.  Every case but e2e also runs tools/copy_yardstick.py in a child process and reports ``copy_equiv_ms``, the
time a device-to-device copy takes for the same number of bytes at the rate measured there.  Device and comparator results
are compared with == before anything is reported."""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cet-driven-simulation-for-3d-printing-am-kmc-approach_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cetkmc  # noqa: E402
import origin_ref as OR  # noqa: E402

FIELDS = tuple(f for f in OR.REC_FIELDS if f != "pad")


def _median(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        got = fn()
        t.append(time.perf_counter() - t0)
    return got, 1e3 * float(np.median(t)), 1e3 * min(t)


def _yardstick(rec, L, n_bytes):
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "copy_yardstick.py"), str(L)], capture_output=True,
                             text=True, timeout=120).stdout
        m = re.search(r"copy .*-> ([0-9.]+) TB/s", out)
        rec["copy_TBps"] = float(m.group(1))
        rec["copy_equiv_ms"] = n_bytes / (rec["copy_TBps"] * 1e12) * 1e3
    except Exception as ex:        # noqa: BLE001 -- the yardstick needs torch; the rest of the record stands without it
        rec["copy_yardstick_error"] = repr(ex)


def _state(L, seed):
    rs = np.random.RandomState(seed)
    return np.where(rs.random_sample((L,) * 3) < 0.4, rs.randint(1, 4, (L,) * 3), 0).astype(np.int64)


def _records(L, n, seed):
    rs = np.random.RandomState(seed)
    ev = np.zeros(n, OR.EVENT)
    ev["type"] = rs.randint(0, 4, n)
    ev["pos"] = rs.randint(0, L, (n, 3))
    ev["target"] = rs.randint(0, L, (n, 3))
    return ev


def absorb(L, reps, n_steps=200):
    """the same 200-step call on two handles, one with a map; the map is compared with the comparator fed by the call's log"""
    z, zi = np.zeros((L,) * 3), np.zeros((L,) * 3, np.int64)
    st = _state(L, 7)
    es = []
    for with_map in (False, True):
        e = cetkmc.Engine(L, impurity_c=0.1)
        e.upload(st, z, z, z + 3300.0, zi)
        e.set_option("reserve_batch", n_steps)
        if with_map:
            e.origin_begin()
        es.append(e)
    words, census, seq = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64), 0
    t = ([], [])
    for k in range(reps + 1):
        for w, e in enumerate(es):
            t0 = time.perf_counter()
            r = e.run_steps(k * n_steps, n_steps, 0.0, None, None, None, rng_mode=2, seed=3, thermal_mode=0)
            if k:
                t[w].append(time.perf_counter() - t0)
            assert (r["done"], r["status"]) == (n_steps, 0)
            if w:
                seq = OR.absorb(words, census, r["events"], seq, 1, L)
    assert np.array_equal(es[1].origin_words(), words) and np.array_equal(es[1].origin_census(), census) and es[1].origin_seq() == seq
    for e in es:
        e.close()
    rec = dict(case=f"absorb_L{L}", L=L, reps=reps, n_steps=n_steps, without_map_ms=1e3 * float(np.median(t[0])),
               with_map_ms=1e3 * float(np.median(t[1])), absorb_bytes=64 * n_steps)
    rec["extra_ms"] = rec["with_map_ms"] - rec["without_map_ms"]
    rec["extra_frac"] = rec["extra_ms"] / rec["without_map_ms"]
    _yardstick(rec, L, rec["absorb_bytes"])
    return rec


def profile(L, R, reps):
    z, zi = np.zeros((L,) * 3), np.zeros((L,) * 3, np.int64)
    if R > 1:
        h = cetkmc.Ensemble(L, [cetkmc.default_params(0.1 * (r % 3)) for r in range(R)])
        reps_h = [h.replica(r) for r in range(R)]
    else:
        h = cetkmc.Engine(L)
        reps_h = [h]
    rs = np.random.RandomState(L)
    blk = np.arange(L) // 8
    for r, e in enumerate(reps_h):      # one orientation per 8^3 block, so that the clustering gives about (L / 8)^3 grains
        st = _state(L, 1000 * L + r)
        nb = int(blk[-1]) + 1
        th, ph = (rs.uniform(0, hi, (nb,) * 3)[np.ix_(blk, blk, blk)] * (st != 0) for hi in (np.pi, 2 * np.pi))
        e.upload(st, th, ph, z + 3000.0, zi)
    h.origin_begin()
    n = int(min(L ** 3, 200000))
    for r, e in enumerate(reps_h):
        e.origin_absorb(_records(L, n, 77 * L + r), 1)
        e.origin_absorb(_records(L, n // 2, 78 * L + r), n // 2)
    if R > 1:
        h.analyze(0.5, labels=False)
    else:
        h.clusters(0.5)
    got, prof_ms, prof_min = _median(lambda: h.origin_profile(grains=True, recluster=False), reps)
    t0 = time.perf_counter()
    words = [e.origin_words() for e in reps_h]
    states = [e.download(theta=False, phi=False, T=False)["state"] for e in reps_h]
    lab = np.zeros((R, L, L, L), np.int32)
    if R > 1:
        h._ck(h.lib.cetkmc_ensemble_analysis_data(h.h, None, None, None, lab.ctypes.data, None, None))
    else:
        h._ck(h.lib.cetkmc_cluster_labels(h.h, lab.ctypes.data))
    t_down = time.perf_counter() - t0
    t0 = time.perf_counter()
    want = [OR.profile(words[r], states[r], lab[r], int(lab[r].max())) for r in range(R)]
    t_ref = time.perf_counter() - t0
    for r in range(R):
        lay = {k: (got["layers"][k][r] if R > 1 else got["layers"][k]) for k in FIELDS}
        gr = got["grains"][r] if R > 1 else got["grains"]
        assert all(np.array_equal(lay[k], want[r][0][k]) and np.array_equal(gr[k], want[r][1][k]) for k in FIELDS), r
    h.close()
    nvox = R * L ** 3
    rec = dict(case=(f"profile_ensemble_L{L}_R{R}" if R > 1 else f"profile_single_L{L}"), L=L, R=R, reps=reps, profile_ms=prof_ms,
               profile_ms_min=prof_min, profile_route_ms=1e3 * (t_down + t_ref), download_ms=1e3 * t_down, numpy_profile_ms=1e3 * t_ref,
               profile_bytes=13 * nvox, profile_GBps=13 * nvox / (prof_ms * 1e-3) / 1e9,
               grains=int(sum(len(w[1]) for w in want)), recorded=int(sum(int((w != 0).sum()) for w in words)))
    rec["profile_speedup"] = rec["profile_route_ms"] / rec["profile_ms"]
    _yardstick(rec, min(L, 256), rec["profile_bytes"])
    return rec


def e2e(L, n_steps, reps=1):
    import tempfile
    import kmc_simulation
    cwd = os.getcwd()
    rec = dict(case=f"e2e_L{L}", L=L, n_steps=n_steps)
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            for name, kw in (("warmup", {}), ("plain_s", {}), ("origin_s", dict(origin_metrics=True))):
                t0 = time.perf_counter()
                kmc_simulation.run_kmc(L=L, n_steps=n_steps if name != "warmup" else 40, impurity_c=0.1, output_prefix=name + "_0", **kw)
                rec[name] = time.perf_counter() - t0
        finally:
            os.chdir(cwd)
    del rec["warmup"]
    rec["overhead"] = rec["origin_s"] / rec["plain_s"] - 1.0
    return rec


CASES = {"absorb_L128": lambda reps: absorb(128, reps), "profile_ensemble_L30_R64": lambda reps: profile(30, 64, reps),
         "profile_ensemble_L128_R16": lambda reps: profile(128, 16, reps), "profile_single_L256": lambda reps: profile(256, 1, reps),
         "e2e_L30": lambda reps: e2e(30, 2000), "e2e_L128": lambda reps: e2e(128, 1000)}


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
