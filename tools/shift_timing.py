"""cetkmc_shift against the route the library offered before it: download the five fields, shift them with NumPy
(tests/shift_ref.py), upload them again -- on the SAME handle.  Prints one JSON line per case and, with --out, writes the list to a
file (profiles/shift.json).

    python tools/shift_timing.py [--reps 10] [--only NAME ...] [--out profiles/shift.json]

Cases: a single handle at 256^3 and an ensemble of R = 16 replicas at L = 128, each shifted by (-8, 0, 0) (a recoated layer:
whole planes move) and by (0, 3, -5) (a moving frame: every row moves, the byte rows misaligned).  Per case, after one warm-up of
each route and alternating the two routes --reps times: ``device_event_ms`` (the time between two hipEvents around the call's
device work, cetkmc_time_shift; the ensemble: ONE cetkmc_ensemble_shift call for all replicas), ``device_wall_ms`` and ``host_wall_ms`` (host clock
around the whole call / the whole download + NumPy + upload), each as median, minimum and maximum, and the bytes_h2d / bytes_d2h
either route added to cetkmc_counters.  ``field_bytes`` is what the move reads and writes at the least, 2 * 26 B per voxel (three
f64 fields and two byte fields, each read once and written once); ``copy_equiv_ms`` the time a device-to-device copy of that
many bytes takes at the rate tools/copy_yardstick.py measures in a child process.  The device route goes through a spare and back:
``moved_bytes`` = 2 * field_bytes + the old state read once more for the counts, and ``moved_GBps_over_whole_call`` divides that by
the event time, which also covers the interface rebuild, the unit vectors and the copy of the counts.  Before anything is reported the two routes' fields are compared with ==."""
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
import shift_ref as SR  # noqa: E402

FILL = dict(fill_state=0, fill_T=2800.0, T_mode="value", fill_theta=0.0, fill_phi=0.0)


def _lattice(L, seed):
    rs = np.random.RandomState(seed)
    st = np.where(rs.random_sample((L,) * 3) < 0.4, rs.randint(1, 5, (L,) * 3), 0).astype(np.int64)
    return st, rs.uniform(0, np.pi, (L,) * 3) * (st != 0), rs.uniform(0, 2 * np.pi, (L,) * 3) * (st != 0), rs.uniform(2800.0, 3600.0, (L,) * 3), \
        (st == 3).astype(np.int64)


def _stats(t):
    t = 1e3 * np.asarray(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def _moved(handles):
    c = [h.counters() for h in handles]
    return sum(x["bytes_h2d"] for x in c), sum(x["bytes_d2h"] for x in c)


def _host_route(e, d):
    out, _ = SR.shift_fields(e.download(defects=True), d, **FILL)
    e.upload(out["state"], out["theta"], out["phi"], out["T"], out["defects"])


def _yardstick(rec, L, n_bytes):
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "copy_yardstick.py"), str(L)], capture_output=True,
                             text=True, timeout=120).stdout
        m = re.search(r"copy .*-> ([0-9.]+) TB/s", out)
        rec["copy_TBps"] = float(m.group(1))
        rec["copy_equiv_ms"] = n_bytes / (rec["copy_TBps"] * 1e12) * 1e3
    except Exception as ex:        # noqa: BLE001 -- the yardstick needs torch; the rest of the record stands without it
        rec["copy_yardstick_error"] = repr(ex)


def case(L, R, d, reps):
    if R > 1:
        h = cetkmc.Ensemble(L, [cetkmc.default_params(0.1) for _ in range(R)])
        lats = [h.replica(r) for r in range(R)]
    else:
        h = cetkmc.Engine(L, impurity_c=0.1)
        lats = [h]
    for r, e in enumerate(lats):
        e.upload(*_lattice(L, 10 * L + r))
    # the two routes give the same fields (checked once, on lattice 0, from the same start)
    start = lats[0].download(defects=True)
    lats[0].shift(d, **FILL)
    by_device = lats[0].download(defects=True)
    lats[0].upload(start["state"], start["theta"], start["phi"], start["T"], start["defects"])
    _host_route(lats[0], d)
    by_host = lats[0].download(defects=True)
    assert all(by_device[k].tobytes() == by_host[k].tobytes() for k in by_device)
    ev, wall_d, wall_h, moved_d, moved_h = [], [], [], [], []
    for k in range(reps + 1):
        b0 = _moved(lats)
        t0 = time.perf_counter()
        ms = h.time_shift([dict(d=d, **FILL)] * R)[1] if R > 1 else h.time_shift(d, **FILL)[1]      # ONE call: cetkmc_ensemble_shift
        t1 = time.perf_counter()
        b1 = _moved(lats)
        for e in lats:
            _host_route(e, d)
        t2 = time.perf_counter()
        b2 = _moved(lats)
        if k:                                  # the first round is the warm-up of both routes
            ev.append(ms * 1e-3)
            wall_d.append(t1 - t0)
            wall_h.append(t2 - t1)
            moved_d.append((b1[0] - b0[0], b1[1] - b0[1]))
            moved_h.append((b2[0] - b1[0], b2[1] - b1[1]))
    h.close()
    nvox = R * L ** 3
    rec = dict(case=f"{'ensemble' if R > 1 else 'single'}_L{L}_R{R}_d{'_'.join(str(x) for x in d)}", L=L, R=R, d=list(d), reps=reps,
               device_event_ms=_stats(ev), device_wall_ms=_stats(wall_d), host_wall_ms=_stats(wall_h),
               device_bytes_h2d=int(moved_d[-1][0]), device_bytes_d2h=int(moved_d[-1][1]),
               host_bytes_h2d=int(moved_h[-1][0]), host_bytes_d2h=int(moved_h[-1][1]), field_bytes=2 * 26 * nvox)
    rec["speedup_wall"] = rec["host_wall_ms"]["median"] / rec["device_wall_ms"]["median"]
    # what the kernels move at the least: every field into the spare and back (2 x field_bytes) and the old state once more for
    # the counts; the event time also covers the interface rebuild, the unit vectors and the copy of the counts
    rec["moved_bytes"] = 2 * rec["field_bytes"] + nvox
    rec["moved_GBps_over_whole_call"] = rec["moved_bytes"] / (rec["device_event_ms"]["median"] * 1e-3) / 1e9
    _yardstick(rec, min(L, 256), rec["field_bytes"])
    return rec


CASES = {"single_256_layer": lambda reps: case(256, 1, (-8, 0, 0), reps), "single_256_frame": lambda reps: case(256, 1, (0, 3, -5), reps),
         "ensemble_128x16_layer": lambda reps: case(128, 16, (-8, 0, 0), reps), "ensemble_128x16_frame": lambda reps: case(128, 16, (0, 3, -5), reps)}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", nargs="*", choices=sorted(CASES), help="a subset of the cases")
    ap.add_argument("--out", default=None, help="write the records to this JSON list")
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: at least 10 repetitions")
    out = []
    for name in a.only or list(CASES):
        rec = CASES[name](a.reps)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)
