"""The selection trees at exact event boundaries, bit for bit: the device against tests/select_ref.py fed with the device's
own bits.

Every other selection test draws uniforms that land inside an event's interval and compares sums at RATE_RTOL = 1e-11
(device libm and glibc differ by a few ulp), so a reduction that adds in another order or a descent that uses > for >= is
invisible to it.  Here the comparator (written from DESIGN.md section 3) is built from what the device itself hands out --
cetkmc_enumerate_events: every leaf rate in reference order, cetkmc_row_sums: the row level, cetkmc_rate_sweep: the total --
so every comparison is ==, and the picks sit one ulp below, on and one ulp above every threshold base + sum(left) / cum of
the descents, plus 0, the total, one ulp above it and twice the total:

(a) the device's row sums, counts and total are the canonical tree over its own leaf rates;
(b) cetkmc_select(r) (k_select) names the comparator's event at every such r;
(c) the batched kernels (k_select_apply, its ensemble form, k_select_pend) form r = u * total on the device: a u with
    u * total == threshold is searched among t / total and its six neighbours; the logged event, totals[0] and min_margin
    are the comparator's.

Lattices: random (all four event kinds), cold top (zero-rate deposition events beside positive ones), melt pool (rates
over 150 decades: runs of bit-equal thresholds).
"""
import functools

import numpy as np
import pytest

import select_ref
from helpers import dep_species, oracle_lattice, random_lattice

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.15
SEED = 11                     # counter generator seed of the rng_mode 1 runs
ENUM_SIZES = (5, 13, 33, 64)
ROW_SIZES = (86, 171, 256, 264, 344)       # block trees of 2, 4 and 8 leaves per thread, two-leaf row tree above 256
KINDS = ("random", "cold_top", "melt_pool")
CAT = select_ref.CATEGORY_OF_TYPE
FIELDS = ("type", "pos", "target", "atom", "dep_rank", "rate")


# ---- lattices -------------------------------------------------------------------------------------------------------
def cold_top(L, seed=5):
    """Plane L-1 empty, its half j < L/2 at 1000 K: the deposition rate nu_dep * exp(-(T_melt - T) / (kT T)) underflows to
    exactly 0.0 there, and the candidates still count as events.  The other half is at 3690 K (rate 3e6, of the size of
    the attachment and diffusion rates below; at 3000 K the rate would underflow to 0.0 as well and no positive leaf
    would stand beside the zero ones).  I0 = 0 (no nucleation), sparse atoms below: rows and voxels without events."""
    rs = np.random.RandomState(seed + L)
    state = np.zeros((L, L, L), np.uint8)
    n_atoms = max(3, min(L ** 3 // 40, 800))
    idx = np.stack([rs.randint(0, L - 1, n_atoms), rs.randint(0, L, n_atoms), rs.randint(0, L, n_atoms)], axis=1)
    state[idx[:, 0], idx[:, 1], idx[:, 2]] = rs.choice([1, 2, 3, 4], n_atoms, p=[0.6, 0.15, 0.2, 0.05])
    atom = (state != 0) & (state != 4)
    theta = np.where(atom, rs.uniform(0, np.pi, (L, L, L)), 0.0)
    phi = np.where(atom, rs.uniform(0, 2 * np.pi, (L, L, L)), 0.0)
    T = np.full((L, L, L), 3000.0)
    T[L - 1] = 3690.0
    T[L - 1, np.arange(L) < L / 2, :] = 1000.0
    return (state, theta, phi, T, np.zeros((L, L, L), np.uint8)), {"I0": 0.0}


def melt_pool(L, seed=3):
    """synthetic.planes (atoms below k = L/4, temperature ramp T_sub .. T_melt along k) plus sprinkled atoms, as
    test_large_L_two_chunks_per_row builds it: rates from 1e-150 to 1e13."""
    from cetkmc import synthetic
    st, th, ph, T, df = synthetic.planes(L, 0, L, seed=seed)
    rs = np.random.RandomState(9 + L)
    n = max(4, L * L // 17)
    idx = rs.randint(0, L, (n, 3))
    st[idx[:, 0], idx[:, 1], idx[:, 2]] = rs.randint(1, 5, n)
    return (st, th, ph, T, df), None


@functools.lru_cache(maxsize=None)
def lattice(kind, L):
    """((state, theta, phi, T, defects), parameter tweak or None); state and defects uint8, as upload_planes takes them."""
    if kind == "cold_top":
        return cold_top(L)
    if kind == "melt_pool":
        return melt_pool(L)
    st, th, ph, T, df = random_lattice(L, 100 + L, fill=0.2)
    return (st.astype(np.uint8), th, ph, T, df.astype(np.uint8)), None


def make_engine(kind, L, n_slabs=1):
    import cetkmc
    lat, tweak = lattice(kind, L)
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in (tweak or {}).items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params, n_slabs=n_slabs)
    e.upload_planes(0, L, *lat)
    return e


def comparator_of(e):
    """select_ref.SelectRef over the device's own enumerated events; (ref, events)."""
    ev, n = e.enumerate_events()
    assert n == len(ev)
    return select_ref.SelectRef(ev["type"], ev["pos"], ev["rate"], e.L), ev


_CASES = {}


def device_case(kind, L):
    """One resident engine per enumerated lattice, its events and its comparator, shared by (a) and (b)."""
    if (kind, L) not in _CASES:
        e = make_engine(kind, L)
        e.rate_sweep()
        ref, ev = comparator_of(e)
        _CASES[kind, L] = (e, ref, ev)
    return _CASES[kind, L]


_ROW_CASES = {}


def row_case(L):
    """Row level only (no enumeration): the melt pool at a large size, the device's row sums and the tree above them."""
    if L not in _ROW_CASES:
        e = make_engine("melt_pool", L)
        info = e.rate_sweep()
        rsum, rcnt = e.row_sums()
        _ROW_CASES[L] = (e, info, select_ref.RowTree(rsum, rcnt, L))
    return _ROW_CASES[L]


# ---- (a) the device's sums have the canonical shape ---------------------------------------------------------------------
def assert_canonical_sums(e, ref, tag):
    total, n_events, n_dep = e.rate_sweep()
    rsum, rcnt = e.row_sums()
    L = e.L
    assert np.array_equal(rcnt.reshape(3 * L, L), ref.rowcnt), (tag, "row counts", np.argwhere(rcnt.reshape(3 * L, L) != ref.rowcnt)[:4])
    bad = np.argwhere(rsum.reshape(3 * L, L) != ref.rowsum)
    assert len(bad) == 0, (tag, "row sums: the device's are not the canonical tree over its enumerated rates", len(bad), bad[:4],
                           [(float(rsum.reshape(3 * L, L)[b, j]).hex(), float(ref.rowsum[b, j]).hex()) for b, j in bad[:4]])
    assert n_events == ref.n_events and n_dep == int(ref.blockcnt[3 * (L - 1)]), (tag, n_events, n_dep)
    assert total == ref.total, (tag, "total", float(total).hex(), float(ref.total).hex())


@pytest.mark.parametrize("L", ENUM_SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_device_sums_are_the_canonical_tree(kind, L):
    """Row sums, counts and total of sweep_variant 0, 1 and 4 (and of a 3-slab handle at L = 13) == the comparator's sums
    over the rates cetkmc_enumerate_events returned."""
    e, ref, ev = device_case(kind, L)
    for v in (0, 1, 4):
        e.set_option("sweep_variant", v)
        assert_canonical_sums(e, ref, f"{kind} L={L} sweep_variant {v}")
        ev2, _ = e.enumerate_events()
        assert ev2.tobytes() == ev.tobytes(), (kind, L, v, "enumerated events depend on the sweep variant")
    if L == 13:
        e3 = make_engine(kind, L, n_slabs=3)
        assert_canonical_sums(e3, ref, f"{kind} L={L} 3 slabs")
        ev3, _ = e3.enumerate_events()
        assert ev3.tobytes() == ev.tobytes()
        e3.close()


@pytest.mark.parametrize("L", ROW_SIZES)
def test_device_total_is_the_canonical_tree_over_its_row_sums(L):
    e, (total, n_events, n_dep), tree = row_case(L)
    assert n_events == tree.n_events and n_dep == int(tree.blockcnt[3 * (L - 1)])
    assert total == tree.total, (L, float(total).hex(), float(tree.total).hex())


def test_melt_pool_has_runs_of_equal_thresholds():
    """The generator's purpose, checked on the comparator: consecutive thresholds of one descent that are bit-equal (a
    rate absorbed by the sum in front of it), and zero-rate events beside positive ones in the cold top."""
    e, ref, ev = device_case("melt_pool", 13)
    assert equal_threshold_runs(ref, np.arange(len(ev))) > 0
    e, ref, ev = device_case("cold_top", 13)
    dep = ev["type"] == 0
    assert (ev["rate"][dep] == 0.0).any() and (ev["rate"][dep] > 0.0).any()


def equal_threshold_runs(ref, indices):
    runs = 0
    for m in indices:
        t = [float(v) for _, v in ref.path_to(m).thresholds]
        runs += sum(a == b for a, b in zip(t, t[1:]))
    return runs


# ---- (b) cetkmc_select on every boundary --------------------------------------------------------------------------------
def boundary_events(ref, n_events, seed):
    """Every event where there are at most 400; otherwise 300 seeded-random ones plus the first and last event of the
    lattice, of a block and of a row that follows an event-free row."""
    if n_events <= 400:
        return np.arange(n_events)
    idx = list(select_ref.event_sample(n_events, 300, seed))
    first_of_row = np.cumsum(ref.rowcnt.ravel()) - ref.rowcnt.ravel()
    rows = ref.rowcnt.ravel()
    L = ref.L
    blocks = np.flatnonzero(ref.blockcnt > 0)
    b = int(blocks[len(blocks) // 2])
    after_gap = [q for q in np.flatnonzero(rows > 0) if q % L and rows[q - 1] == 0]
    spans = [(0, n_events), (int(first_of_row[b * L]), int(first_of_row[b * L] + ref.blockcnt[b]))]
    if after_gap:
        q = int(after_gap[len(after_gap) // 2])
        spans.append((int(first_of_row[q]), int(first_of_row[q] + rows[q])))
    for lo, hi in spans:
        idx += [lo, hi - 1]
    return np.unique(np.array(idx))


def _record(x):
    """The compared fields of a cetkmc_event (ctypes struct) or of a record of an event array, as plain values."""
    get = (lambda f: x[f]) if isinstance(x, np.void) else (lambda f: getattr(x, f))
    return {f: tuple(int(v) for v in get(f)) if f in ("pos", "target") else (float(get(f)) if f == "rate" else int(get(f)))
            for f in FIELDS}


def assert_event(got, want, tag):
    g, w = _record(got), _record(want)
    assert g == w, (tag, "device", g, "comparator", w)


def check_selects(e, ref, ev, picks, want, tag):
    for r, m in zip(picks, want):
        assert_event(e.select(r), ev[m], f"{tag} r={float(r).hex()}")


@pytest.mark.parametrize("kind,L", [(k, L) for k in KINDS for L in ENUM_SIZES] + [("cold_top", 264)])
def test_select_on_every_boundary(kind, L):
    """cetkmc_select(r) for r one ulp below, on and one ulp above every threshold of the sampled descents, and for 0, the
    total, one ulp above it and twice the total (fallback to the last event): ties go left, zero-rate events are
    reachable only through a tie, an equal-threshold run yields its first event.  ("cold_top", 264): the two-leaf voxel
    tree with an event list small enough to enumerate."""
    e, ref, ev = device_case(kind, L)
    assert len(ev) < 100_000 or L <= 64
    thr = select_ref.thresholds_of(ref, boundary_events(ref, len(ev), L))
    picks = select_ref.picks_around([t for level in select_ref.LEVELS for t in thr[level]], ref.total)
    want = [ref.select(r).index for r in picks]
    assert want[-1] == len(ev) - 1                 # a pick above the total falls back to the last event
    print(f"{kind} L={L}: {len(ev)} events, thresholds per level {[len(thr[lv]) for lv in select_ref.LEVELS]}, {len(picks)} picks")
    variants = (0, 1, 4) if L <= 64 else (1,)
    for v in variants:
        e.set_option("sweep_variant", v)
        e.rate_sweep()
        check_selects(e, ref, ev, picks, want, f"{kind} L={L} sweep_variant {v}")
    if L == 13:
        e3 = make_engine(kind, L, n_slabs=3)
        e3.rate_sweep()
        check_selects(e3, ref, ev, picks, want, f"{kind} L={L} 3 slabs")
        e3.close()


@pytest.mark.parametrize("L", ROW_SIZES)
def test_select_row_on_block_and_row_boundaries(L):
    """The large block and row trees: (plane, category, row) of cetkmc_select(r) against the comparator's descent over the
    device's row sums, around at most 300 block-level and row-level thresholds."""
    e, (total, n_events, n_dep), tree = row_case(L)
    rows = np.flatnonzero(tree.rowcnt.ravel() > 0)
    rs = np.random.RandomState(L)
    chosen = list(rs.choice(rows, 60, replace=False)) + [rows[0], rows[-1]]
    seen = {}
    for q in chosen:
        for level, t in tree.path_to_row(int(q) // (3 * L), (int(q) // L) % 3, int(q) % L).thresholds:
            seen.setdefault(float(t), level)
    thr = list(seen)[:300]
    assert {seen[t] for t in thr} == {"block", "row"}
    picks = select_ref.picks_around(thr, tree.total)
    for r in picks:
        got, want = e.select(r), tree.select_row(r)
        assert (got.pos[0], int(CAT[got.type]), got.pos[1]) == (want.i, want.c, want.j), \
            (L, float(r).hex(), "device", tuple(got.pos), got.type, "comparator", (want.i, want.c, want.j))


# ---- (c) the batched kernels at a boundary ------------------------------------------------------------------------------
def craft_u(t, total):
    """A uniform in [0, 1) with u * total == t, among t / total and its neighbours up to 3 ulp away; None without one."""
    u0 = np.float64(t) / np.float64(total)
    cands, up, dn = [u0], u0, u0
    for _ in range(3):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        cands += [up, dn]
    for u in cands:
        if 0.0 <= u < 1.0 and u * np.float64(total) == t:
            return float(u)
    return None


def crafted_thresholds(ref_thresholds, total, per_level, seed):
    """per_level thresholds of every level that has any, each with a reachable u, walking a seeded shuffle of the
    candidates: [(level, t, [(pick, u) of t's reachable variants])].  Fails instead of thinning: at least three quarters of
    the thresholds tried must be reachable (on random doubles the share is 1.00 for t of the total's magnitude and 0.92
    six decades below it), and every level must keep at least 3."""
    rs = np.random.RandomState(seed)
    out, tried, reached = [], 0, 0
    for level, vals in ref_thresholds.items():
        kept = 0
        for q in rs.permutation(len(vals)):
            if kept == per_level:
                break
            t = vals[q]
            tried += 1
            if craft_u(t, total) is None:
                continue
            reached += 1
            kept += 1
            out.append((level, t, [(r, craft_u(r, total)) for r in select_ref.boundary_picks(t) if craft_u(r, total) is not None]))
        assert kept >= min(3, per_level), (level, "reachable thresholds", kept, "of", len(vals))
    assert reached >= 0.75 * tried, ("reachable share", reached, tried)
    return out


def expected_species(ev, rng_mode, u_np, L, step=0):
    """The species a logged deposition carries: rng_mode 0 draws one uniform per candidate (the chosen one's is
    u_np[dep_rank] on a call's first step), rng_mode 1 takes the counter uniform keyed by the site."""
    from oracle import oracle
    if rng_mode == 0:
        return dep_species(u_np[int(ev["dep_rank"])], IMPURITY_C)
    return dep_species(oracle.counter_uniform(SEED, step, int(ev["pos"][1]) * L + int(ev["pos"][2])), IMPURITY_C)


def assert_logged_event(got, want, rng_mode, u_np, L, tag):
    w = want.copy()
    if w["type"] == 0:
        w["atom"] = expected_species(w, rng_mode, u_np, L)
    assert_event(got, w, tag)


@pytest.mark.parametrize("kind,L,n_slabs", [("random", 13, 1), ("cold_top", 13, 1), ("melt_pool", 13, 1), ("random", 64, 1),
                                            ("melt_pool", 64, 1), ("random", 20, 3), ("cold_top", 20, 3)])
def test_fused_select_apply_on_boundaries(oracle_mod, kind, L, n_slabs):
    """k_select_apply: one run_steps call of 2 steps on a freshly uploaded lattice, u_pick[0] crafted; rng_mode 1 and 0."""
    e = make_engine(kind, L, n_slabs)
    e.rate_sweep()
    ref, ev = comparator_of(e)
    thr = select_ref.thresholds_of(ref, boundary_events(ref, len(ev), L))
    crafted = crafted_thresholds(thr, ref.total, 3, L)
    assert len(crafted) == 12
    lat = lattice(kind, L)[0]
    rs = np.random.RandomState(L)
    u_np = rs.random_sample(2 * (L * L + 2))
    for level, t, variants in crafted:
        for r, u in variants:
            want = ev[ref.select(r).index]
            margin = ref.margin(r)
            for rng_mode in (1, 0):
                e.upload_planes(0, L, *lat)
                res = e.run_steps(0, 2, 0.0, np.array([u, 0.37]), None, u_np, rng_mode=rng_mode, seed=SEED, thermal_mode=0)
                tag = f"{kind} L={L} slabs={n_slabs} {level} threshold {float(t).hex()} r={float(r).hex()} rng_mode {rng_mode}"
                assert res["done"] == 2 and res["status"] == 0, tag
                assert res["totals"][0] == ref.total, (tag, "total")
                assert_logged_event(res["events"][0], want, rng_mode, u_np, L, tag)
                assert res["min_margin"] <= margin, (tag, "min_margin", res["min_margin"], margin)
            # a one-step call reports the margin of its only pick: exactly 0.0 on the upper end of the chosen interval
            e.upload_planes(0, L, *lat)
            res = e.run_steps(0, 1, 0.0, np.array([u]), None, u_np, rng_mode=1, seed=SEED, thermal_mode=0)
            assert res["done"] == 1 and res["totals"][0] == ref.total, tag
            assert_logged_event(res["events"][0], want, 1, u_np, L, tag)
            assert res["min_margin"] == margin, (tag, "min_margin of a one-step call", res["min_margin"], margin)
    e.close()


def test_deferred_select_on_boundaries():
    """k_select_pend: L = 136, 3 steps so that step 0 launches its selection alone.  No enumeration at this size: block-
    and row-level thresholds over the device's row sums, (plane, category, row) of the logged event."""
    L = 136
    e = make_engine("melt_pool", L)
    total, _, _ = e.rate_sweep()
    rsum, rcnt = e.row_sums()
    tree = select_ref.RowTree(rsum, rcnt, L)
    assert total == tree.total
    rows = np.flatnonzero(tree.rowcnt.ravel() > 0)
    rs = np.random.RandomState(L)
    thr = {"block": {}, "row": {}}
    for q in rs.choice(rows, 40, replace=False):
        for level, t in tree.path_to_row(int(q) // (3 * L), (int(q) // L) % 3, int(q) % L).thresholds:
            thr[level].setdefault(float(t), None)
    crafted = crafted_thresholds({k: [np.float64(t) for t in v] for k, v in thr.items()}, tree.total, 4, L)
    assert len(crafted) == 8
    lat = lattice("melt_pool", L)[0]
    u_np = rs.random_sample(8)
    for level, t, variants in crafted:
        for r, u in variants:
            want = tree.select_row(r)
            e.upload_planes(0, L, *lat)
            e.reset_counters()
            res = e.run_steps(0, 3, 0.0, np.array([u, 0.37, 0.73]), None, u_np, rng_mode=1, seed=SEED, thermal_mode=0)
            tag = f"L={L} {level} threshold {float(t).hex()} r={float(r).hex()}"
            assert res["done"] == 3 and e.counters()["deferred_steps"] > 0, tag
            assert res["totals"][0] == tree.total, (tag, "total")
            got = res["events"][0]
            assert (got["pos"][0], int(CAT[got["type"]]), got["pos"][1]) == (want.i, want.c, want.j), (tag, got)
    e.close()


@pytest.mark.parametrize("kind,L", [("random", 13), ("cold_top", 13), ("random", 64), ("melt_pool", 64)])
def test_ensemble_select_apply_on_boundaries(oracle_mod, kind, L):
    """The ensemble form of k_select_apply: R = 48 copies of one lattice, replica r gets the crafted u of threshold r // 3,
    variant r % 3 (below, on, above), one call of one step, rng_mode 0.  The call has no event log: the lattice each
    replica holds afterwards must be the uploaded one with the comparator's event applied."""
    import cetkmc
    R = 48
    lat, tweak = lattice(kind, L)
    e = make_engine(kind, L)
    e.rate_sweep()
    ref, ev = comparator_of(e)
    params = e.params
    e.close()
    thr = select_ref.thresholds_of(ref, boundary_events(ref, len(ev), L))
    crafted = crafted_thresholds(thr, ref.total, 4, L)
    assert len(crafted) == 16
    ens = cetkmc.Ensemble(L, [params] * R)
    rs = np.random.RandomState(L)
    u_np = rs.random_sample((R, L * L + 2))
    picks = np.zeros(R)
    u_pick = np.zeros(R)
    for r in range(R):
        level, t, _ = crafted[r // 3]
        pick = select_ref.boundary_picks(t)[r % 3]
        u = craft_u(pick, ref.total)
        if u is None:                          # this variant has no uniform: an ordinary pick, compared all the same
            u = float(rs.random_sample())
            pick = np.float64(u) * ref.total
        picks[r], u_pick[r] = pick, u
        ens.replica(r).upload_planes(0, L, *lat)
    res = ens.run(0, 1, 0.0, u_pick=u_pick.reshape(R, 1), u_np=u_np, rng_mode=0, thermal_mode=0)
    base = oracle_lattice(oracle_mod, lat, IMPURITY_C, tweak)
    n_dep = int(ref.blockcnt[3 * (L - 1)])
    for r in range(R):
        tag = f"{kind} L={L} replica {r} ({crafted[r // 3][0]} threshold, variant {r % 3}) r={float(picks[r]).hex()}"
        assert (res["done"][r], res["status"][r]) == (1, 0), tag
        assert res["totals"][r][0] == ref.total, (tag, "total")
        assert res["min_margin"][r] == ref.margin(picks[r]), (tag, "min_margin", res["min_margin"][r], ref.margin(picks[r]))
        want = ev[ref.select(picks[r]).index]
        oe = oracle_mod.Event()
        oe.type, oe.rate, oe.dep_rank = int(want["type"]), float(want["rate"]), int(want["dep_rank"])
        oe.pos[:], oe.target[:] = [int(x) for x in want["pos"]], [int(x) for x in want["target"]]
        oe.atom = expected_species(want, 0, u_np[r], L) if want["type"] == 0 else int(want["atom"])
        o = oracle_mod.Lattice(base.state, base.theta, base.phi, base.T, base.defects, impurity_c=IMPURITY_C)
        o.apply(oe, 0.0 + (3.141592653589793 - 0.0) * u_np[r][n_dep], 0.0 + (6.283185307179586 - 0.0) * u_np[r][n_dep + 1], False)
        d = ens.replica(r).download(T=False)
        for f in ("state", "theta", "phi"):
            assert np.array_equal(d[f], getattr(o, f)), (tag, f, "event", want, np.argwhere(d[f] != getattr(o, f))[:4])
    ens.close()
