"""bench.py --dump-outputs: the files it writes (names, float32 / float64 only, the 64 MB budget, a seeded lattice sample
that does not change from call to call), on a stand-in for the engine -- no GPU needed."""
import glob
import os

import numpy as np

import bench
from cetkmc.engine import EVENT_DTYPE


class FakeEngine:
    """download_planes of a fixed random lattice; owns planes i0..i1 of an L^3 lattice."""

    def __init__(self, L, i0, i1):
        self.L, self.i0, self.i1 = L, i0, i1
        rs = np.random.RandomState(7)
        shape = (i1 - i0, L, L)
        self.f = dict(state=rs.randint(0, 5, shape).astype(np.uint8), defects=rs.randint(0, 2, shape).astype(np.uint8),
                      theta=rs.random_sample(shape), phi=rs.random_sample(shape), T=rs.random_sample(shape))

    def download_planes(self, i_begin, i_end, **kw):
        assert (i_begin, i_end) == (self.i0, self.i1)
        return {k: v.copy() for k, v in self.f.items() if kw.get(k)}


def _result(L, n, seed=0):
    rs = np.random.RandomState(seed)
    ev = np.zeros(n, EVENT_DTYPE)
    ev["type"] = rs.randint(0, 4, n)
    ev["pos"] = rs.randint(0, L, (n, 3))
    ev["target"] = np.where(rs.random_sample((n, 1)) < 0.5, -1, rs.randint(0, L, (n, 3)))
    ev["rate"], ev["theta"], ev["phi"] = rs.random_sample(n), rs.random_sample(n), rs.random_sample(n)
    return dict(events=ev, n_events=rs.randint(1, 1000, n), totals=rs.random_sample(n), done=n, status=0, np_used=2 * n,
                q_used=1, nucleation_count=3, full_sweeps=n)


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(os.path.join(d, "*.npy"))}


def test_dump_outputs_files_budget_and_sample(tmp_path):
    L, n = 96, 50                                   # 884 736 owned voxels: more than the sample
    eng = FakeEngine(L, 0, L)
    r = _result(L, n)
    info = bench.dump_outputs(str(tmp_path / "a"), eng, r, 45, L)
    bench.dump_outputs(str(tmp_path / "b"), eng, r, 45, L)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == sorted(b) and len(a) == info["files"]
    assert all(np.array_equal(a[k], b[k]) for k in a)                # the sample is fixed
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert sum(os.path.getsize(f) for f in glob.glob(str(tmp_path / "a" / "*.npy"))) <= bench.DUMP_BYTES_MAX
    assert np.array_equal(a["step_index"], np.arange(45, 45 + n)) and a["run_result"][0] == n
    assert np.array_equal(a["events_pos"], r["events"]["pos"]) and np.array_equal(a["totals"], r["totals"])
    assert len(a["lattice_index"]) == bench.DUMP_SAMPLE_VOXELS and np.all(np.diff(a["lattice_index"]) > 0)
    for prefix in ("lattice", "site"):
        idx = a[f"{prefix}_index"].astype(np.int64)
        for f in ("state", "defects", "theta", "phi", "T"):
            assert np.array_equal(a[f"{prefix}_{f}"], eng.f[f].reshape(-1)[idx]), (prefix, f)
    sites = {tuple(p) for p in r["events"]["pos"]} | {tuple(t) for t in r["events"]["target"] if t[0] >= 0}
    assert {tuple(np.unravel_index(i, (L, L, L))) for i in a["site_index"].astype(np.int64)} == sites


def test_dump_outputs_rank_slab_and_step_cap(tmp_path, monkeypatch):
    """A rank dumps its own planes (global indices); past DUMP_STEPS_MAX steps only the last ones are kept."""
    monkeypatch.setattr(bench, "DUMP_STEPS_MAX", 8)
    L, n = 16, 30
    eng = FakeEngine(L, 4, 12)
    r = _result(L, n, seed=1)
    info = bench.dump_outputs(str(tmp_path), eng, r, 100, L)
    a = _load(tmp_path)
    assert info["steps_logged"] == 8 and np.array_equal(a["step_index"], np.arange(122, 130))
    assert np.array_equal(a["events_rate"], r["events"]["rate"][-8:])
    assert np.array_equal(a["lattice_index"], np.arange(4 * L * L, 12 * L * L))
    assert np.all((a["site_index"] >= 4 * L * L) & (a["site_index"] < 12 * L * L))
