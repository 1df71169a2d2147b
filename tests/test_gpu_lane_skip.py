"""Option table_lane_skip: the census-free tiles that request a lane's rate-table entries only where its class bytes can use
them, against the same tiles with every lane's entries, bit for bit, and each against the oracle.

With the option on (default) a wave of a census-free tile (sweep_table_tile(), options fused_tiles 1 / 2) requests the class
bytes of its two items first and then, per lane, the 64 B of table entries only if lane_needs_values() holds for the lane's own
8 class bytes: some voxel is empty or is an atom with a non-zero count.  A lane of defects, outside voxels and unexposed atoms
(every byte 0x00 or 0x02) loads nothing and holds zeros.  Which lanes those are changes from step to step: the upkeep of an
applied event rewrites class bytes (ifc_store()), and the next launch must then load a lane it skipped before.

Lattices.  kfill = 34 at both sizes (L = 129: the first size on the path, odd, so the last row pair is half empty; L = 136),
that is kfill = 2 (mod 8): lanes 0..3 of a row (k < 32) are solid and unexposed, the two top atom layers k = 32, 33 sit alone in
lane 4 under the melt.  On top of that, as helpers.face_lattice: atoms strewn everywhere (a strewn atom inside the solid is just
another unexposed atom; one in the melt makes its lane live) and atoms on the faces.  Each size runs a second lattice with a
few wholly solid rows (state[i, j, :] = 1: every lane of that half-wave is masked) and one wholly solid interior plane.

The skipped-to-live transition is steered.  A top-layer atom with all its bonds never diffuses in 45 steps (its rate is some 1e-12
of the total), so each lattice holds two LONE top-layer atoms: the 8 neighbours in their own layer are removed and the row above
them is empty, which leaves them 3 bonds and about 1e-6 of the total.  The pick uniform of each call's first step (a deferred
step) is replaced by one computed from the ORACLE's own sums that selects a diffusion of such an atom (steer()).  Before that
step lane 3 (k = 24..31) of the atom's row is skipped -- checked on the oracle's state with a restatement of the class bytes --
and the diffusion empties (i, j, 33), which exposes the atom two below it, (i, j, 31): lane 3 is live in the next launch.

Coverage is counted from the oracle's log and states, never the engine's; the inputs were checked with the oracle alone on the
CPU (counts in the tests' docstrings)."""
import os

import numpy as np
import pytest

from helpers import FOUR_KIND_PARAMS, assert_call_matches_oracle, batch_calls, count_deferred, deferred_coverage, is_deferred, oracle_lattice
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DEFECT_FRACTION = 0.05
BATCHES = (24, 21)                 # steps 0..44: temperature updates at steps 20 and 40, one inside each call
N_ATOMS = 6000
KFILL = 34
SEED = {129: 146, 136: 153}        # helpers.face_lattice's 17 + L
EV_DIFF = 1


def lone_sites(L):
    """(i, j) of the two lone top-layer atoms: interior rows, one per call"""
    return [(20, 31), (L - 30, 2 * (L // 3))]


def lattice(L, seed, solid):
    """uint8 planes as Engine.upload_planes takes them: synthetic.planes with kfill = 34 + helpers.face_lattice's strewn and face
    atoms (+ solid rows and a solid plane) + the lone top-layer atoms"""
    from cetkmc import synthetic
    st, th, ph, T, df = synthetic.planes(L, 0, L, seed=seed, fill_frac=KFILL / L + 1e-9)
    assert st[:, :, KFILL - 1].all() and not st[:, :, KFILL:].any()
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, L, (N_ATOMS, 3))
    st[idx[:, 0], idx[:, 1], idx[:, 2]] = rs.randint(1, 5, N_ATOMS)
    for f in range(8):
        st[0, rs.randint(L), rs.randint(L)] = 1 + f % 3
        st[L - 1, rs.randint(L), rs.randint(L)] = 1 + f % 3
        st[rs.randint(L), 0, rs.randint(L)] = 1 + f % 3
        st[rs.randint(L), L - 1, rs.randint(L)] = 1 + f % 3
    if solid:
        for (i, j) in ((5, 6), (5, 7), (40, L - 1), (77, 0), (L - 2, 64), (64, 65)):
            st[i, j, :] = 1
        st[L // 2 + 3, :, :] = 1
    k = KFILL - 1
    for (i, j) in lone_sites(L):
        st[i, j, :KFILL] = 1                               # W atoms below, no defect in the column
        st[i, j, KFILL:] = 0                               # nothing in the melt of this row: the lone atom is the row's diffusion sum
        for (di, dj) in ((1, 1), (1, -1), (-1, 1), (-1, -1), (2, 0), (-2, 0), (0, 2), (0, -2)):
            st[i + di, j + dj, k] = 0
    return st, th, ph, T, df


def lane_skipped(oracle_mod, state, i, j, lane):
    """restated class bytes of voxels 8 lane .. 8 lane + 7 of row (i, j): every voxel is non-empty and no atom among them has an
    empty neighbour (bytes 0x00 / 0x02: lane_needs_values() is false)"""
    L = state.shape[0]
    for k in range(8 * lane, min(8 * lane + 8, L)):
        if state[i, j, k] == 0:
            return False
        nb = oracle_mod.neighbors(i, j, k, L)
        if state[i, j, k] != 4 and (state[nb[:, 0], nb[:, 1], nb[:, 2]] == 0).any():
            return False
    return True


def steer(o, site):
    """A pick uniform under which the oracle's selection on its present lattice takes a diffusion of the atom at `site`: blocks
    are ordered plane by plane (deposition, diffusion, empty), rows by j; the atom's events are all but the row's whole diffusion
    sum (its one other exposed atom, (i, j, 32), has 12 bonds), so the middle of the row's interval is far inside them."""
    i, j, k = site
    sw = o.sweep()
    r = sw["blocksum"][:3 * i + 1].sum() + sw["rowsum"][i, 1, :j].sum() + 0.5 * sw["rowsum"][i, 1, j]
    u = r / sw["total"]
    ev = o.select_tree(sw["blocksum"], sw["blockcnt"], sw["rowsum"], sw["rowcnt"], u * sw["total"])
    assert ev is not None and ev.type == EV_DIFF and tuple(ev.pos) == site, (site, ev and ev.astuple())
    return u


def top_diffusions(calls, logs):
    """deferred steps of the oracle's log whose event is a diffusion out of the top atom layer"""
    return [tuple(int(x) for x in ro["events"][x]["pos"]) for (step0, n, *_), ro in zip(calls, logs) for x in range(ro["done"])
            if is_deferred(step0, n, x) and int(ro["events"][x]["type"]) == EV_DIFF and int(ro["events"][x]["pos"][2]) == KFILL - 1]


def _engine(L, lat, skip):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.set_option("table_lane_skip", skip)
    e.upload_planes(0, L, *lat)
    e.set_prev_state(None)
    return e


def _observed(e, r):
    """the event log, the totals, the candidate counts, the stream positions and the final fields of a call (test_gpu_fused_tiles)"""
    d = e.download(defects=True)
    return (r["done"], r["status"], r["np_used"], r["q_used"], r["nucleation_count"], r["full_sweeps"], r["totals"].tobytes(),
            r["events"].tobytes(), r["n_events"].tobytes()) + tuple(d[k].tobytes() for k in sorted(d))


def run_oracle_call(oracle_mod, o, L, c, call, steered):
    """one call on the oracle, its first pick steered to the c-th lone atom; returns (the call as run, the oracle's result)"""
    from cetkmc import synthetic
    step0, n, u_pick, u_def, u_np = call
    i, j = lone_sites(L)[c]
    assert is_deferred(step0, n, 0)
    assert lane_skipped(oracle_mod, o.state, i, j, 3) and o.state[i, j, KFILL - 3] in (1, 2, 3), (i, j)
    kw = dict(rng_mode=1, seed=5, thermal_mode=2, q_planes=synthetic.laser_planes(L, step0, n))
    at = o
    if step0 % 20 == 0:         # the step selects behind a temperature update: steer on a copy that has made run_steps' update
        at = oracle_mod.Lattice(o.state, o.theta, o.phi, o.T, o.defects, impurity_c=IMPURITY_C)
        at.params, at.prev_state = o.params, o.prev_state.copy()
        at.thermal_laser(1e-6, kw["q_planes"][0], scrub_nan=True)
    u_pick = u_pick.copy()
    u_pick[0] = steer(at, (i, j, KFILL - 1))
    steered.append((i, j, KFILL - 1))
    ro = o.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
    assert not lane_skipped(oracle_mod, o.state, i, j, 3) or o.state[i, j, KFILL - 1] != 0      # (refilled only by a later event)
    return (step0, n, u_pick, u_def, u_np), kw, ro


def _run_case(oracle_mod, L, solid):
    lat, calls = lattice(L, SEED[L], solid), batch_calls(BATCHES)
    o = oracle_lattice(oracle_mod, lat, IMPURITY_C, FOUR_KIND_PARAMS)
    engines = {s: _engine(L, lat, s) for s in (1, 0)}
    logs, ran, steered = [], [], []
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        for c, call in enumerate(calls):
            call, kw, ro = run_oracle_call(oracle_mod, o, L, c, call, steered)
            step0, n, u_pick, u_def, u_np = call
            ran.append(call)
            logs.append(ro)
            seen = {}
            for s, e in engines.items():
                rg = e.run_steps(step0, n, DEFECT_FRACTION, u_pick, u_def, u_np, **kw)
                seen[s] = _observed(e, rg)
                assert_call_matches_oracle(e, o, rg, ro, RATE_RTOL, tag=f"L={L} call {c}, table_lane_skip {s}")
            for q, (x, y) in enumerate(zip(seen[1], seen[0])):
                assert x == y, f"L={L} call {c}: item {q} of the observed state differs between table_lane_skip 1 and 0"
    finally:
        oracle_mod.set_threads(1)
    n_def = count_deferred(ran)
    assert n_def == sum(BATCHES) - len(BATCHES) - 2          # every step but each call's last and the one before each update
    for e in engines.values():
        cnt = e.counters()
        assert cnt["deferred_steps"] == n_def and cnt["incremental_steps"] == 0, cnt
        e.close()
    assert all(ro["done"] == c[1] and ro["status"] == 0 for ro, c in zip(logs, ran))
    cov = deferred_coverage(L, ran, logs, DEFECT_FRACTION)
    top = top_diffusions(ran, logs)
    print(f"L={L} solid={solid} deferred-step coverage (oracle log): {cov}, diffusions out of the top layer: {top}")
    assert min(cov["kinds"]) >= 1, cov                       # deposition, diffusion, nucleation, attachment: all on deferred steps
    assert len(top) >= 1 and set(steered) <= set(top), (steered, top)
    return cov, top


def test_lane_skip_L129(oracle_mod):
    """Odd L, 1049 tiles.  Oracle's log, 41 deferred steps: kinds [17, 6, 4, 14] (deposition, diffusion, nucleation, attachment); 2
    diffusions of a lone top-layer atom at k = 33, (20, 31) at step 0 and (99, 86) at step 24, each to (i, j - 1, 34)."""
    _run_case(oracle_mod, 129, False)


def test_lane_skip_L129_solid_rows(oracle_mod):
    """+ six wholly solid rows and the solid plane 67.  Oracle's log: kinds [17, 3, 3, 18]; the same 2 diffusions out of the top layer."""
    _run_case(oracle_mod, 129, True)


def test_lane_skip_L136(oracle_mod):
    """1156 tiles.  Oracle's log, 41 deferred steps: kinds [17, 4, 2, 18]; 2 diffusions of a lone top-layer atom at k = 33, (20, 31) at
    step 0 and (106, 90) at step 24."""
    _run_case(oracle_mod, 136, False)


def test_lane_skip_L136_solid_rows(oracle_mod):
    """+ six wholly solid rows and the solid plane 71.  Oracle's log: kinds [17, 3, 3, 18]; the same 2 diffusions out of the top layer."""
    _run_case(oracle_mod, 136, True)
