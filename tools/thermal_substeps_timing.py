"""Sub-stepped temperature updates: what one update and the stepping loop cost, on the bench's lattice
(cetkmc.synthetic.planes, the moving source of synthetic.laser_planes).  Every leg is a child process of its own; the legs are
alternated over --rounds.  Prints one JSON line per record and, with --out, appends the list to a file
(profiles/thermal_substeps.json).

    python tools/thermal_substeps_timing.py [--L 256] [--n 17] [--steps 2000] [--rounds 3] [--parent-lib PATH] [--out FILE]

(a) ``update``: one laser + latent-heat update in --n sub-steps from hipEvents (cetkmc_time_thermal, --reps single updates,
    their median) -- legs ``plain`` (option substep_block = 1: n launches of the existing kernel), ``S2``, ``S3``, ``S4``
    (k_thermal_sub with that many sub-steps per launch), ``direct`` (thermal_substeps = 1 and n updates in one event pair: the
    existing kernel n times, latent term and scrub in each) and, with --parent-lib, ``parent`` (n cetkmc_thermal_laser calls of
    the parent's library, host wall clock: its source-plane copy and synchronisation are inside).  ``us`` per update.
(b) ``loop``: the --steps-step loop (counter uniforms, thermal_mode 2 with latent heat, reserve_batch) -- legs ``parent``,
    ``n1`` (this library, thermal_substeps never set), ``blocked`` and ``plain`` (n = --n).  ``ms`` lists the hipEvent wall times
    of the call (cetkmc_run_result.wall_ms), ``median_ms`` their median; ``parent_spread_ms`` is max - min of the parent's.
With --pmc-leg NAME the process runs that update leg once more, untimed, for a counter run of its own
(rocprofv3 --pmc FETCH_SIZE ... -- python tools/thermal_substeps_timing.py --pmc-leg S4).  No figure is a gate."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cet-driven-simulation-for-3d-printing-am-kmc-approach_amd")
sys.path.insert(0, PKG)

IMPURITY_C, SEED = 0.2, 42
UPDATE_LEGS = ("parent", "direct", "plain", "S2", "S3", "S4")
LOOP_LEGS = ("parent", "n1", "blocked", "plain")
NEW_SYMBOLS = ("cetkmc_set_thermal_substeps", "cetkmc_ensemble_set_thermal_substeps", "cetkmc_get_substep_info", "cetkmc_time_thermal")


def _engine(L, parent=False):
    from cetkmc import _lib
    if parent:      # a library from before sub-stepping: it has none of its symbols
        for k in NEW_SYMBOLS:
            _lib.PROTOTYPES.pop(k, None)
        _lib.STRUCT_MIRRORS.pop("substep_info", None)
    import cetkmc
    from cetkmc import synthetic
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    e.upload_planes(0, L, *synthetic.planes(L, 0, L, seed=SEED))
    e.set_prev_state(None)
    return e


def _configure(e, name, n):
    if name in ("plain", "blocked") or name.startswith("S"):
        e.set_thermal_substeps(n)
        e.set_option("substep_block", 1 if name == "plain" else 0 if name == "blocked" else int(name[1:]))


def update_leg(name, L, n, reps, timed=True):
    from cetkmc import synthetic
    e = _engine(L, parent=name == "parent")
    q = synthetic.laser_planes(L, 0, 20)[0]
    _configure(e, name, n)
    e.thermal_laser(1e-6, q, use_latent=True, scrub_nan=True)          # the plane the timed updates use; warm-up
    us = []
    for _ in range(reps if timed else 1):
        if name == "parent":
            e.sync()
            t0 = time.perf_counter()
            for _ in range(n):
                e.thermal_laser(1e-6 / n, q, use_latent=True, scrub_nan=True)
            us.append((time.perf_counter() - t0) * 1e6)
        elif name == "direct":
            us.append(e.time_thermal(n, laser=True) * 1e3)
        else:
            us.append(e.time_thermal(1, laser=True) * 1e3)
    rec = dict(leg=name, us=float(np.median(us)), us_min=float(min(us)))
    if name not in ("parent", "direct"):
        rec.update(e.substep_info())
    e.close()
    print(json.dumps(rec))


def loop_leg(name, L, n, steps):
    from cetkmc import synthetic
    e = _engine(L, parent=name == "parent")
    e.set_option("reserve_batch", steps)
    _configure(e, name, n)
    kw = dict(rng_mode=2, seed=SEED, thermal_mode=2, use_latent=True, want_logs=False)
    e.run_steps(0, 200, 0.003, None, None, None, q_planes=synthetic.laser_planes(L, 0, 200), **kw)          # warm-up
    r = e.run_steps(200, steps, 0.003, None, None, None, q_planes=synthetic.laser_planes(L, 200, steps), **kw)
    rec = dict(leg=name, done=r["done"], status=r["status"], wall_ms=r["wall_ms"])
    if name in ("blocked", "plain"):
        rec.update(e.substep_info())
    e.close()
    print(json.dumps(rec))


def _children(kind, legs, a, key):
    vals = {n: [] for n in legs}
    last = {}
    for _ in range(a.rounds):
        for n in legs:
            env = dict(os.environ)
            if n == "parent":
                env["CETKMC_LIB"] = os.path.abspath(a.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", f"{kind}:{n}", "--L", str(a.L), "--n", str(a.n),
                                  "--steps", str(a.steps), "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=600)
            if out.returncode:
                raise RuntimeError(f"leg {kind}:{n} failed: {out.stderr[-2000:]}")
            last[n] = json.loads(out.stdout.strip().splitlines()[-1])
            vals[n].append(last[n][key])
    return vals, last


def update(a):
    legs = [n for n in UPDATE_LEGS if n != "parent" or a.parent_lib]
    us, last = _children("update", legs, a, "us")
    rec = dict(case="update", L=a.L, n=a.n, rounds=a.rounds, reps=a.reps)
    for n in legs:
        rec[n] = dict(us=us[n], median_us=float(np.median(us[n])), **{k: v for k, v in last[n].items() if k not in ("leg", "us", "us_min")})
    rec["fastest"] = min((n for n in legs if n not in ("parent", "direct")), key=lambda n: rec[n]["median_us"])
    return rec


def loop(a):
    legs = [n for n in LOOP_LEGS if n != "parent" or a.parent_lib]
    ms, last = _children("loop", legs, a, "wall_ms")
    rec = dict(case="loop", L=a.L, n=a.n, steps=a.steps, rounds=a.rounds)
    for n in legs:
        rec[n] = dict(ms=ms[n], median_ms=float(np.median(ms[n])), **{k: v for k, v in last[n].items() if k not in ("leg", "wall_ms")})
    if "parent" in ms:
        rec["parent_spread_ms"] = max(ms["parent"]) - min(ms["parent"])
        rec["n1_minus_parent_ms"] = rec["n1"]["median_ms"] - rec["parent"]["median_ms"]
    rec["plain_over_blocked"] = rec["plain"]["median_ms"] / rec["blocked"]["median_ms"]
    return rec


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=256)
    ap.add_argument("--n", type=int, default=17)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--what", default="update,loop", help="comma list of update, loop")
    ap.add_argument("--parent-lib", default=None, help="libcetkmc_hip.so built from the parent commit (the 'parent' legs)")
    ap.add_argument("--leg", default=None, help="(internal) KIND:NAME -- run one leg in this process")
    ap.add_argument("--pmc-leg", default=None, choices=UPDATE_LEGS[1:], help="one untimed update of that leg (for a counter run)")
    ap.add_argument("--out", default=None, help="append the records to this JSON list")
    a = ap.parse_args()
    if a.pmc_leg:
        update_leg(a.pmc_leg, a.L, a.n, 1, timed=False)
        sys.exit(0)
    if a.leg:
        kind, name = a.leg.split(":")
        update_leg(name, a.L, a.n, a.reps) if kind == "update" else loop_leg(name, a.L, a.n, a.steps)
        sys.exit(0)
    out = []
    for what in a.what.split(","):
        rec = update(a) if what == "update" else loop(a)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        old = json.load(open(a.out)) if os.path.exists(a.out) else []
        json.dump(old + out, open(a.out, "w"), indent=1)
