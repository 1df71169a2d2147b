"""Replica-ensemble throughput (cetkmc.Ensemble) against the same replicas run one after another through single Engines,
in one process.  Prints one JSON line.

For each (L, R, RNG mode): executed events/s summed over replicas, device us per ensemble step (hipEvents around the
call's launches), host ms per call, the sequential baseline, and the algorithmic sweep traffic 9 B x L^3 x R per step
over the device step time (an L2 / Infinity-Cache figure at these sizes: 64 replicas of 30^3 move ~16 MB per sweep).
Reference mode draws its streams the way run_kmc_ensemble does (per-replica random.random() loops and NumPy streams).
``end_to_end`` rows time the public path, kmc_simulation.run_kmc_ensemble (metrics rows, defect refreshes, CSVs included),
against the same runs through run_kmc one after another."""
import argparse
import json
import os
import sys
import time

import random
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "cet-driven-simulation-for-3d-printing-am-kmc-approach_amd"))
import cetkmc  # noqa: E402
import kmc_simulation  # noqa: E402
import lattice_init  # noqa: E402


def lattices(L, R):
    out = []
    for r in range(R):
        np.random.seed(1000 + r)
        st, th, ph, T, _ = lattice_init.initialize_lattice(lattice_size=L, n_seeds=5, impurity_c=0.1 * (r % 3))
        out.append((st, th, ph, T))
    return out


def one(L, R, mode, steps, seq_cap, scheme="explicit", n_sub=1):
    lat = lattices(L, R)
    params = [cetkmc.default_params(0.1 * (r % 3)) for r in range(R)]
    ens = cetkmc.Ensemble(L, params)
    ens.set_thermal_substeps(n_sub)
    ens.set_thermal_scheme(scheme)
    for r, (st, th, ph, T) in enumerate(lat):
        ens.replica(r).upload(st, th, ph, T, np.zeros_like(st))
    per_step = L * L + 2
    n = steps if mode == "counter" else max(1, min(steps, (1 << 25) // (R * per_step)))
    rs = np.random.RandomState(0)
    pys = [random.Random(r) for r in range(R)]
    nps = [np.random.RandomState(r) for r in range(R)]

    def call(step0):
        t0 = time.perf_counter()
        if mode == "counter":
            res = ens.run(step0, n, np.zeros(R), rng_mode=2, seeds=np.arange(R), thermal_mode=1)
            draw = 0.0
        else:               # as run_kmc_ensemble: each replica's own CPython and NumPy generators
            u_pick = np.array([[pys[r].random() for _ in range(2 * n)] for r in range(R)]).reshape(R, n, 2)[:, :, 0]
            u_np = np.stack([nps[r].random_sample(n * per_step) for r in range(R)])
            draw = time.perf_counter() - t0
            res = ens.run(step0, n, np.zeros(R), u_pick, None, u_np, rng_mode=0, thermal_mode=1)
        return res, time.perf_counter() - t0, draw
    call(0)                                  # warm-up (first launches, allocations)
    calls, events, wall, dev, draw = 3, 0, 0.0, 0.0, 0.0
    for c in range(calls):
        res, w, d = call((c + 1) * n)
        events += int(res["done"].sum())
        wall += w
        dev += res["wall_ms"]
        draw += d
    ens.close()
    step_us = dev * 1e3 / (calls * n)
    # baseline: the same replicas one after another through single Engines (at most seq_cap of them, scaled to R)
    k = min(R, seq_cap)
    t_seq, ev_seq = 0.0, 0
    for r in range(k):
        e = cetkmc.Engine(L, params=params[r])
        e.set_thermal_substeps(n_sub)
        e.set_thermal_scheme(scheme)
        st, th, ph, T = lat[r]
        e.upload(st, th, ph, T, np.zeros_like(st))
        if mode == "counter":
            e.run_steps(0, n, 0.0, None, None, None, rng_mode=2, seed=r, thermal_mode=1)
        else:
            e.run_steps(0, n, 0.0, rs.random_sample(n), None, rs.random_sample(n * per_step), rng_mode=0, thermal_mode=1)
        t0 = time.perf_counter()
        for c in range(calls):
            if mode == "counter":
                out = e.run_steps((c + 1) * n, n, 0.0, None, None, None, rng_mode=2, seed=r, thermal_mode=1)
            else:
                out = e.run_steps((c + 1) * n, n, 0.0, rs.random_sample(n), None, rs.random_sample(n * per_step), rng_mode=0,
                                  thermal_mode=1)
            ev_seq += out["done"]
        t_seq += time.perf_counter() - t0
        e.close()
    seq_rate = ev_seq / t_seq if t_seq > 0 else 0.0
    ens_rate = events / wall
    return dict(L=L, R=R, rng=mode, thermal_scheme=scheme, thermal_substeps=n_sub, steps_per_call=n,
                events_per_s=round(ens_rate, 1), device_us_per_step=round(step_us, 2),
                host_ms_per_call=round(wall * 1e3 / calls, 3), host_draw_ms_per_call=round(draw * 1e3 / calls, 3),
                sequential_events_per_s=round(seq_rate, 1), sequential_replicas_timed=k,
                speedup=round(ens_rate / seq_rate, 2) if seq_rate else None,
                sweep_GBps_L2=round(9.0 * L ** 3 * R / (step_us * 1e-6) / 1e9, 1))


def end_to_end(L, R, mode, n_steps, seq_cap):
    """run_kmc_ensemble vs run_kmc one after another (at most seq_cap of the runs, scaled to R), same configs."""
    cfgs = [dict(impurity_c=0.1 * (r % 3), seed=42 + r, defect_fraction=3e-3, output_prefix=f"e2e_{r}") for r in range(R)]
    seq_kw = dict(mode="B", box=L, thermal_cadence="supersteps") if mode == "counter" else {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        os.chdir(d)
        try:
            out = open(os.devnull, "w")
            old, sys.stdout = sys.stdout, out
            try:
                kmc_simulation.run_kmc_ensemble(cfgs[:1], L, 20, rng=mode)          # warm-up
                t0 = time.perf_counter()
                kmc_simulation.run_kmc_ensemble(cfgs, L, n_steps, rng=mode)
                t_ens = time.perf_counter() - t0
                k = min(R, seq_cap)
                t0 = time.perf_counter()
                for c in cfgs[:k]:
                    kmc_simulation.run_kmc(L=L, n_steps=n_steps, **c, **seq_kw)
                t_seq = (time.perf_counter() - t0) * R / k
            finally:
                sys.stdout = old
        finally:
            os.chdir(cwd)
    return dict(L=L, R=R, rng=mode, n_steps=n_steps, metrics_every=kmc_simulation.METRIC_UPDATE_STEP,
                run_kmc_ensemble_s=round(t_ens, 3), sequential_run_kmc_s=round(t_seq, 3), sequential_runs_timed=k,
                events_per_s=round(R * n_steps / t_ens, 1), sequential_events_per_s=round(R * n_steps / t_seq, 1),
                speedup=round(t_seq / t_ens, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--L", type=int, nargs="*", default=[30, 64])
    ap.add_argument("--R", type=int, nargs="*", default=[1, 8, 16, 64, 256])
    ap.add_argument("--e2e-steps", type=int, default=1000, help="end-to-end rows (L = 30, R = 16 / 64); 0: none")
    ap.add_argument("--modes", nargs="*", default=["counter", "reference"])
    ap.add_argument("--seq-cap", type=int, default=8)
    ap.add_argument("--thermal-scheme", default="explicit", choices=["explicit", "implicit"], help="of the `rows` (ensemble and baseline)")
    ap.add_argument("--thermal-substeps", type=int, default=1, help="of the `rows` (ensemble and baseline)")
    a = ap.parse_args()
    rows = [one(L, R, m, a.steps, a.seq_cap, a.thermal_scheme, a.thermal_substeps) for L in a.L for R in a.R for m in a.modes]
    e2e = [end_to_end(30, R, m, a.e2e_steps, 4) for R in (16, 64) for m in a.modes] if a.e2e_steps > 0 else []
    print(json.dumps(dict(tool="ensemble_throughput", rows=rows, end_to_end=e2e)))


if __name__ == "__main__":
    main()
