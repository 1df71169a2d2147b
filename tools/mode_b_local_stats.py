#!/usr/bin/env python3
"""Mode B against Mode A at equal executed-event counts, for the null-event mode and the local event loop, in one job.

    python tools/mode_b_local_stats.py [--L 64] [--events 48000] [--seeds 8] --out profiles/mode_b_local_stats.json

Runs tools/mode_b_stats.collect() with and without the temperature updates for the null-event mode and for the local loop at
(max_events, horizon_events) = (4, 1), (8, 4), (16, 8) -- what `mode_b_stats.py [--no-thermal] [--local-events K
--local-horizon X]` runs one at a time -- and writes the eight summaries (mode_b_stats.summarize) with the seconds each took.
GPU box only."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mode_b_stats  # noqa: E402

SETTINGS = ((0, 0.0), (4, 1.0), (8, 4.0), (16, 8.0))

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=64)
    ap.add_argument("--events", type=int, default=48000)
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    res = dict(L=a.L, events=a.events, seeds=a.seeds, runs=[])
    for thermal in (False, True):
        for K, hor in SETTINGS:
            t0 = time.time()
            rows = mode_b_stats.collect(L=a.L, n_events=a.events, seeds=range(a.seeds), box=8, null_events=True,
                                        thermal_cadence="events", thermal_updates=thermal, local_events=K, local_horizon=hor or 1.0)
            s = mode_b_stats.summarize(rows)
            res["runs"].append(dict(thermal_updates=thermal, mode="local" if K else "null_events", local_events=K, local_horizon=hor,
                                    seconds=time.time() - t0, summary=s))
            print(thermal, K, hor, {c: round(v["rel_diff"], 4) for c, v in s.items() if "rel_diff" in v}, flush=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1, default=str)
