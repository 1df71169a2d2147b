"""Option apply_in_sweep: a deferred step launches its selection alone and the next sweep launch applies the event in an
extra workgroup (k_select_pend -> k_sweep_stream_apply -> k_plane_reduce with the stale rows' patch).  Every result must
equal the immediate select + apply path bit for bit: per-step logs, counters, row sums and the downloaded lattice."""
import numpy as np
import pytest

from helpers import APPLY_IN_SWEEP_BATCHES, FOUR_KIND_PARAMS, batch_calls, count_deferred, is_deferred
from helpers import face_lattice as _lattice
from helpers import step_uniforms as _uniforms

pytestmark = pytest.mark.gpu


def _run(L, lat, calls, on, rng_mode=1, defect_fraction=0.05, tweak=None):
    """calls: (step0, n, u_pick, u_def, u_np); returns everything observable after each call.  The deferred-step counter
    must say which path ran: every eligible step with the option on, none with it off."""
    import cetkmc
    from cetkmc import synthetic
    params = cetkmc.default_params(0.2)
    for k, v in (tweak or {}).items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=0.2, params=params)
    e.set_option("apply_in_sweep", int(on))
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    out = []
    for step0, n, u_pick, u_def, u_np in calls:
        q = synthetic.laser_planes(L, step0, n)
        r = e.run_steps(step0, n, defect_fraction, u_pick, u_def, u_np, rng_mode=rng_mode, seed=5, thermal_mode=2, q_planes=q)
        d = e.download(defects=True)
        info = e.rate_sweep()           # row / block sums of the lattice the call left
        rs, rc = e.row_sums()
        out.append((r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["full_sweeps"],
                    r["totals"].tobytes(), r["events"].tobytes(), r["n_events"].tobytes(), info, rs.tobytes(), rc.tobytes())
                   + tuple(d[k].tobytes() for k in sorted(d)))
    deferred = e.counters()["deferred_steps"]
    e.close()
    assert deferred == (count_deferred(calls) if on else 0), (on, deferred, count_deferred(calls))
    return out


def _compare(L, lat, calls, **kw):
    a = _run(L, lat, calls, True, **kw)
    b = _run(L, lat, calls, False, **kw)
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[:6] == y[:6], (k, x[:6], y[:6])
        assert x == y, f"call {k}: results differ"
    return a


def _events(out):
    """the per-call event logs of _run's result (the executed steps of each call)"""
    from cetkmc.engine import EVENT_DTYPE
    return [np.frombuffer(o[7], dtype=EVENT_DTYPE) for o in out]


def _deferred_kinds(calls, out):
    """events of each kind on deferred steps and, of the diffusions among them, those whose sites lie in different rows"""
    kinds, diff_rows = [0, 0, 0, 0], 0
    for (step0, n, *_), ev in zip(calls, _events(out)):
        for x in range(len(ev)):
            if is_deferred(step0, n, x):
                t = int(ev["type"][x])
                kinds[t] += 1
                diff_rows += int(t == 1 and tuple(ev["pos"][x][:2]) != tuple(ev["target"][x][:2]))
    return kinds, diff_rows


@pytest.mark.parametrize("L", [256, 200])
def test_apply_in_sweep_bit_identical_across_offsets(L):
    """Batches starting and ending at many offsets modulo 20 (temperature updates inside and at the edges), 1-step
    batches, defect injection (defect_fraction 0.05), depositions in plane L-1 and events near the faces."""
    lat = _lattice(L, 17 + L, 6000)
    calls, s = [], 0
    for k, n in enumerate((7, 1, 13, 1, 20, 26, 2, 19, 3, 1)):
        u_pick, u_def, u_np = _uniforms(100 + k, n, 2 * n + 2)
        calls.append((s, n, u_pick, u_def, u_np))
        s += n
    out = _compare(L, lat, calls)
    assert all(o[0] == c[1] and o[1] == 0 for o, c in zip(out, calls))


def test_apply_in_sweep_stream_shortage_and_continuation():
    """Reference stream (rng_mode 0): the batch stops when u_np runs out (status 2); the continuation resumes from the
    step it stopped at.  Both paths stop at the same step with the same lattice."""
    L = 160
    lat = _lattice(L, 5, 3000)
    n = 30
    u_pick, u_def, u_np = _uniforms(7, n, 9 * (L * L + 2))
    out_a = _run(L, lat, [(4, n, u_pick, u_def, u_np)], True, rng_mode=0)
    out_b = _run(L, lat, [(4, n, u_pick, u_def, u_np)], False, rng_mode=0)
    assert out_a == out_b
    done = out_a[0][0]
    assert out_a[0][1] == 2 and done < n
    # continuation: a fresh call from the stopped step with a fresh stream
    u_np2 = np.random.RandomState(8).random_sample(40 * (L * L + 2))
    calls = [(4, n, u_pick, u_def, u_np), (4 + done, 12, u_pick[done:], u_def[done:], u_np2)]
    a = _run(L, lat, calls, True, rng_mode=0)
    b = _run(L, lat, calls, False, rng_mode=0)
    assert a == b and a[1][1] == 0 and a[1][0] == 12


def test_apply_in_sweep_termination():
    """A lattice without events terminates at the first selection (status 1) on both paths."""
    L = 144
    st, th, ph, T, df = _lattice(L, 3, 10)
    st[:] = 4
    u_pick, u_def, u_np = _uniforms(9, 10, 22)
    a = _run(L, (st, th, ph, T, df), [(1, 10, u_pick, u_def, u_np)], True)
    b = _run(L, (st, th, ph, T, df), [(1, 10, u_pick, u_def, u_np)], False)
    assert a == b and a[0][1] == 1 and a[0][0] == 0


def test_apply_in_sweep_diffusion_events():
    """A lattice with many W/Re/C atoms beside empty voxels, a cool field and I0 lowered to 1e11 (at the default 5e13 every
    chosen event of this lattice is a nucleation): diffusion moves (two changed sites, stale rows around both) are among
    the events applied inside a sweep.  The oracle gives 4 diffusions, 6 nucleations and 18 attachments for these inputs,
    3 of the diffusions on deferred steps and between different rows."""
    L = 192
    st, th, ph, T, df = _lattice(L, 11, 40000)
    T[:] = np.minimum(T, 1500.0)
    calls = []
    for k, n in enumerate((19, 9)):
        u_pick, u_def, u_np = _uniforms(30 + k, n, 2 * n + 2)
        calls.append((0 if k == 0 else 19, n, u_pick, u_def, u_np))
    out = _compare(L, (st, th, ph, T, df), calls, tweak=FOUR_KIND_PARAMS)
    assert out[0][0] == 19 and out[1][0] == 9
    ev = np.concatenate(_events(out))
    moved = ev[(ev["type"] == 1) & ((ev["pos"][:, 0] != ev["target"][:, 0]) | (ev["pos"][:, 1] != ev["target"][:, 1]))]
    assert len(moved) >= 2, ev["type"]
    kinds, diff_rows = _deferred_kinds(calls, out)
    assert diff_rows >= 2, (kinds, diff_rows)


@pytest.mark.parametrize("L", [256, 200])
def test_apply_in_sweep_four_event_kinds(L):
    """The batches of the offsets test plus one of 37 steps with I0 = 1e11: depositions, diffusions, nucleations and
    attachments are all applied inside a sweep (the same inputs run against the oracle in
    test_gpu_deferred_apply_vs_oracle.py, where the oracle's log gives at least 7 of each kind on deferred steps)."""
    lat = _lattice(L, 17 + L, 6000)
    calls = batch_calls(APPLY_IN_SWEEP_BATCHES + (37,))
    out = _compare(L, lat, calls, tweak=FOUR_KIND_PARAMS)
    assert all(o[0] == c[1] and o[1] == 0 for o, c in zip(out, calls))
    kinds, diff_rows = _deferred_kinds(calls, out)
    assert min(kinds) >= 3 and diff_rows >= 2, (kinds, diff_rows)
