"""bench.py: a plain run plans no extra measurement, --full plans all that fit the configuration, the --no-... options narrow
--full (no GPU); on the GPU, a plain and a --full run time the same steps and the plain line carries none of the extras."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import ROOT

EXTRA_KEYS = ("cpu_baseline", "pcie_inclusive", "phases", "sweep_recompute", "incremental_exact", "mode_b", "mode_b_null_events",
              "mode_b_null_events_stationary_T")


def _extras(argv, N=1, world=1, L=256, config5=False):
    return bench.extras(bench.parse_args(argv), N, world, L, config5)


def test_plain_run_plans_no_extras():
    assert bench.parse_args([]).full is False
    for argv in ([], ["--gpus", "1", "--steps", "20", "--warmup", "5"], ["--no-mode-b"], ["--extras-multi"]):
        assert _extras(argv) == set()
    assert _extras(["--gpus", "8"], N=8, world=8, L=512, config5=True) == set()


def test_full_plans_every_extra_that_fits():
    assert _extras(["--full"]) == set(bench.EXTRAS)
    for name, off in bench.EXTRAS.items():
        if off:
            assert _extras(["--full", "--" + off.replace("_", "-")]) == set(bench.EXTRAS) - {name}
    # what fits: no 512^3 leg beside another lattice edge, no Mode B boxes in an edge that 8 does not divide
    assert _extras(["--full", "--L", "64"], L=64) == set(bench.EXTRAS) - {"hbm_512"}
    assert _extras(["--full", "--L", "60"], L=60) == set(bench.EXTRAS) - {"hbm_512", "mode_b"}
    # several ranks: Mode B, the phase table and the transfers; the single-GPU legs only on request
    multi = {"phases", "mode_b", "event_overhead", "pcie_inclusive"}
    assert _extras(["--full", "--gpus", "2"], N=2, world=2) == multi
    assert _extras(["--full", "--gpus", "2", "--extras-multi"], N=2, world=2) == multi | {"incremental_exact"}
    assert _extras(["--full", "--config5"], config5=True) == set(bench.EXTRAS) - {"live_traffic", "cpu_baseline", "hbm_512"}
    assert _extras(["--full", "--force-dist"]) == set(bench.EXTRAS) - {"live_traffic"}


def _bench(tmp_path, tag, *more):
    out = tmp_path / tag
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--L", "32", "--steps", "20", "--warmup", "5",
                        "--dump-outputs", str(out), *more], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}


@pytest.mark.gpu
def test_plain_and_full_runs_time_the_same_steps(tmp_path):
    plain, dump_p = _bench(tmp_path, "plain")
    # (the rocprofv3 child runs measure the sweep's traffic at the flagship size; they are not what this test is about)
    full, dump_f = _bench(tmp_path, "full", "--full", "--no-live-traffic")
    for line in (plain, full):
        assert line["metric"] == "kmc_events_per_sec" and line["unit"] == "executed events/s" and line["dtype"] == "f64"
        assert line["higher_is_better"] is True and line["steps"] == 20 and line["warmup"] == 5
        assert line["value"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"])
        assert "extras_errors" not in line, line["extras_errors"]
    assert plain["full"] is False and plain["extras"] == []
    assert not [k for k in EXTRA_KEYS if k in plain] and plain["roofline"]["hbm_512"] is None
    assert plain["roofline"]["launches_timed"] > 0                     # the timed steps' own sweep timing stays
    assert full["full"] is True and set(full["extras"]) == set(bench.EXTRAS) - {"live_traffic", "hbm_512"}
    assert all(k in full for k in EXTRA_KEYS) and full["cpu_baseline"]["parity_first_steps"] is True
    # the same steps of the same trajectory: 40 lead-in steps, 5 warm-up steps, then the timed ones
    assert sorted(dump_p) == sorted(dump_f) and len(dump_p) == plain["dump_outputs"]["files"]
    assert np.array_equal(dump_p["step_index"], np.arange(45, 65))
    for k in dump_p:
        assert np.array_equal(dump_p[k], dump_f[k]), k
