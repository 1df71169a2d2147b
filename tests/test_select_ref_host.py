"""tests/select_ref.py (the comparator of tests/test_gpu_select_edges.py, written from DESIGN.md section 3) pinned to the
oracle, on the event boundaries: no GPU.

Both are fed the oracle's own ``enumerate()`` list, so every comparison is ==: the row sums, block sums and total of
``Lattice.sweep()``, and the event ``Lattice.select_tree`` names for picks one ulp below, on and one ulp above every
threshold base + sum(left) / cum of the sampled descents, for 0, the total, one ulp above it and twice the total.  (The
oracle's own consistency test skips picks closer than 1e-9 to a boundary.)"""
import glob
import os

import numpy as np
import pytest

import select_ref
from helpers import GOLDEN, load, oracle_lattice
from test_gpu_select_edges import IMPURITY_C, equal_threshold_runs, lattice

EVENT_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "events_*.npz")))
GENERATED = [("cold_top", 13), ("melt_pool", 13)]


def _oracle_case(oracle_mod, name):
    if isinstance(name, tuple):
        lat, tweak = lattice(*name)
        return oracle_lattice(oracle_mod, lat, IMPURITY_C, tweak)
    z = load(name)
    return oracle_mod.Lattice(z["state"], z["theta"], z["phi"], z["T"], z["defects"], impurity_c=float(z["impurity_c"]))


@pytest.mark.parametrize("name", EVENT_CASES + GENERATED, ids=lambda n: n if isinstance(n, str) else f"{n[0]}_L{n[1]}")
def test_comparator_vs_oracle_on_boundaries(oracle_mod, name):
    lat = _oracle_case(oracle_mod, name)
    L = lat.L
    ev, n_dep = lat.enumerate()
    sw = lat.sweep()
    ref = select_ref.SelectRef(ev["type"], ev["pos"], ev["rate"], L)
    assert np.array_equal(ref.rowcnt.reshape(L, 3, L), sw["rowcnt"])
    assert np.array_equal(ref.rowsum.reshape(L, 3, L), sw["rowsum"], equal_nan=True)
    assert np.array_equal(ref.blockcnt, sw["blockcnt"])
    assert np.array_equal(ref.blocksum, sw["blocksum"], equal_nan=True)
    assert np.array_equal(ref.total, sw["total"], equal_nan=True)
    assert (ref.n_events, int(ref.blockcnt[3 * (L - 1)])) == (sw["n_events"], sw["n_dep"]) == (len(ev), n_dep)
    if not np.isfinite(sw["total"]) or len(ev) == 0:
        return
    thr = select_ref.thresholds_of(ref, select_ref.event_sample(len(ev), 400, L))
    picks = select_ref.picks_around([t for level in select_ref.LEVELS for t in thr[level]], ref.total)
    for r in picks:
        got = ref.select(r)
        want = lat.select_tree(sw["blocksum"], sw["blockcnt"], sw["rowsum"], sw["rowcnt"], float(r))
        g = ev[got.index]
        assert (int(g["type"]), tuple(g["pos"]), tuple(g["target"]), int(g["dep_rank"]), float(g["rate"])) == \
               (want.type, tuple(want.pos), tuple(want.target), want.dep_rank, want.rate), (name, float(r).hex())
        assert (got.i, got.c, got.j, got.k) == (g["pos"][0], select_ref.CATEGORY_OF_TYPE[g["type"]], g["pos"][1], g["pos"][2])
    assert ref.select(picks[-1]).index == len(ev) - 1            # above the total: the last event


def test_path_to_is_the_descent_select_makes():
    """path_to(m) (steered by the event) and select(r) (steered by a pick inside that event's interval) walk the same
    nodes: same thresholds, base and running sum."""
    rs = np.random.RandomState(1)
    L = 3
    pos, typ, rate = [], [], []
    for i in range(L):
        for c, t in ((0, 0), (1, 1), (2, 3)):
            for j in range(L):
                for k in range(L):
                    for _ in range(rs.randint(0, 3)):
                        pos.append((i, j, k)), typ.append(t), rate.append(rs.uniform(0.5, 2.0))
    ref = select_ref.SelectRef(typ, pos, rate, L)
    on_end = 0
    for m in range(len(rate)):
        p = ref.path_to(m)
        r = p.p_cum - 0.25 * rate[m]
        s = ref.select(r)
        assert s.index == p.index == m
        assert [(a, float(b)) for a, b in s.thresholds] == [(a, float(b)) for a, b in p.thresholds]
        assert s.base == p.base and s.p_cum == p.p_cum
        assert ref.margin(r) == min(abs(r - (p.p_cum - rate[m])), abs(p.p_cum - r)) / ref.total
        # the upper end of the interval: margin exactly 0 where the pick stays with this event (a tree-summed threshold
        # above may round below this running sum and send the pick to the next event)
        on_end += ref.select(p.p_cum).index == m
        assert ref.select(p.p_cum).index != m or ref.margin(p.p_cum) == 0.0
    assert on_end > len(rate) // 2


def test_generators_make_their_edges(oracle_mod):
    """The melt pool yields descents with bit-equal consecutive thresholds; the cold top zero-rate deposition events beside
    positive ones, a zero-sum row that holds events beside a positive one."""
    lat = _oracle_case(oracle_mod, ("melt_pool", 13))
    ev, _ = lat.enumerate()
    ref = select_ref.SelectRef(ev["type"], ev["pos"], ev["rate"], 13)
    assert equal_threshold_runs(ref, np.arange(len(ev))) > 0
    lat = _oracle_case(oracle_mod, ("cold_top", 13))
    ev, _ = lat.enumerate()
    dep = ev["type"] == 0
    assert (ev["rate"][dep] == 0.0).any() and (ev["rate"][dep] > 0.0).any()
    ref = select_ref.SelectRef(ev["type"], ev["pos"], ev["rate"], 13)
    b = 3 * 12
    zero_rows = (ref.rowsum[b] == 0.0) & (ref.rowcnt[b] > 0)
    assert zero_rows.any() and (ref.rowsum[b] > 0.0).any()
