"""tests/origin_ref.py, the comparator of the origin map, pinned without a GPU on 2^3 and 3^3 cases whose words, census and
records are written out by hand: every event type, overwrite order within and across calls, LEFT then refill, skipped
records (idle, null, a diffusion without a target), ties of a group broken by code and then by position, empty records, and
the identities between the plane records and the words."""
import numpy as np

import origin_ref as OR

I64MAX = np.iinfo(np.int64).max


def _rec(n_occ=0, n_by=(0, 0, 0, 0), n_unrec=0, n_left=0, ord_sum=0, ord_min=I64MAX, ord_max=-1, birth=I64MAX):
    return (n_occ, tuple(n_by), n_unrec, n_left, ord_sum, ord_min, ord_max, birth, 0)


def _tuples(recs):
    return [(int(r["n_occ"]), tuple(int(x) for x in r["n_by"]), int(r["n_unrec"]), int(r["n_left"]), int(r["ord_sum"]),
             int(r["ord_min"]), int(r["ord_max"]), int(r["birth"]), int(r["pad"])) for r in recs]


def _three_calls():
    """the 2^3 map every test below reads: (words, census, seq) after three calls"""
    L = 2
    words, census = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64)
    ev = OR.make_events([(0, (0, 0, 0), None),              # 0 dep
                         (2, (0, 0, 1), None),              # 1 nuc
                         (3, (1, 0, 0), (0, 0, 0)),         # 2 att (target = the source neighbour: not written)
                         (1, (0, 0, 0), (1, 1, 1)),         # 3 diff: (0,0,0) LEFT, (1,1,1) HOP
                         (-1, (0, 0, 0), None),             # 4 idle: skipped, its ordinal passes
                         (-2, (1, 1, 1), None),             # 5 null
                         (1, (0, 0, 1), (-1, -1, -1)),      # 6 diffusion without a target
                         (0, (0, 0, 0), None)])             # 7 dep: refills the voxel that was left
    seq = OR.absorb(words, census, ev, 0, 1, L)
    assert seq == 8
    assert words.reshape(-1).tolist() == [(8 << 3) | 1, (2 << 3) | 2, 0, 0, (3 << 3) | 3, 0, 0, (4 << 3) | 4]
    assert census.tolist() == [[2, 1, 1, 0, 0], [0, 0, 0, 1, 1]]
    # second call, two records per ordinal: nuc and att of ordinal 8 meet on one voxel (the larger code stays), the dep of
    # ordinal 9 overwrites the nucleation of the first call
    ev = OR.make_events([(2, (1, 1, 0), None), (3, (1, 1, 0), (1, 1, 1)), (0, (0, 0, 1), None), (-1, (0, 0, 0), None)])
    seq = OR.absorb(words, census, ev, seq, 2, L)
    assert seq == 10
    assert words.reshape(-1).tolist() == [65, (10 << 3) | 1, 0, 0, 27, 0, (9 << 3) | 3, 36]
    assert census.tolist() == [[3, 1, 1, 0, 0], [0, 0, 1, 2, 1]]
    # third call: the attached voxel hops on
    seq = OR.absorb(words, census, OR.make_events([(1, (1, 0, 0), (1, 0, 1))]), seq, 1, L)
    assert seq == 11
    assert words.reshape(-1).tolist() == [65, 81, 0, 0, (11 << 3) | 5, (11 << 3) | 4, 75, 36]
    assert census.tolist() == [[3, 1, 1, 0, 0], [0, 1, 1, 2, 2]]
    return words, census, seq


def test_absorb_by_hand():
    words, census, seq = _three_calls()
    o, c = OR.decode(words)
    assert o.reshape(-1).tolist() == [7, 9, -1, -1, 10, 10, 8, 3] and c.reshape(-1).tolist() == [1, 1, 0, 0, 5, 4, 3, 4]


def test_absorb_is_order_free_within_a_call():
    """later wins as a maximum: one call, or the same records in two halves, or the whole lot with the records of each
    group reversed -- the same words and census"""
    L, n, group = 3, 24, 4
    rs = np.random.RandomState(3)
    rows = []
    for q in range(n):
        t = int(rs.randint(-2, 4))
        pos = tuple(int(x) for x in rs.randint(0, L, 3))
        tgt = tuple(int(x) for x in rs.randint(0, L, 3)) if t in (1, 3) else None
        rows.append((t, pos, tgt))
    ev = OR.make_events(rows)
    a = (np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64))
    assert OR.absorb(a[0], a[1], ev, 5, group, L) == 5 + n // group
    b = (np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64))
    mid = OR.absorb(b[0], b[1], ev[:8], 5, group, L)
    assert OR.absorb(b[0], b[1], ev[8:], mid, group, L) == 5 + n // group
    c = (np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64))
    OR.absorb(c[0], c[1], ev.reshape(-1, group)[:, ::-1], 5, group, L)
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])
    assert a[0].any()


def test_profile_by_hand():
    words, _, _ = _three_calls()
    # voxel (0,0,1) holds a record but is empty (an upload took it away): it counts in nothing; (0,1,0) is occupied without a
    # record; (1,0,0) is empty and LEFT
    state = np.array([1, 0, 2, 0, 0, 1, 3, 1]).reshape(2, 2, 2)
    labels = np.array([1, 2, 1, 0, 3, 3, 3, 0]).reshape(2, 2, 2)       # label 2 and a label of grain 3 sit on empty voxels
    layers, grains = OR.profile(words, state, labels, 4)
    assert _tuples(layers) == [
        _rec(2, (1, 0, 0, 0), 1, 0, 7, 7, 7, (7 << 27) | (1 << 24) | 0),
        _rec(3, (0, 0, 1, 2), 0, 1, 21, 3, 10, (3 << 27) | (4 << 24) | 7)]
    assert _tuples(grains) == [
        _rec(2, (1, 0, 0, 0), 1, 0, 7, 7, 7, (7 << 27) | (1 << 24) | 0),
        _rec(1, (1, 0, 0, 0), 0, 0, 9, 9, 9, (9 << 27) | (1 << 24) | 1),
        _rec(3, (0, 0, 1, 1), 1, 0, 18, 8, 10, (8 << 27) | (3 << 24) | 6),       # the LEFT word of (1,0,0) is no fill: unrecorded
        _rec()]                                                                  # a grain without a voxel: the empty record
    only_layers, none = OR.profile(words, state)
    assert none is None and _tuples(only_layers) == _tuples(layers)
    empty, _ = OR.profile(np.zeros((2,) * 3, np.uint64), np.zeros((2,) * 3, np.int64))
    assert _tuples(empty) == [_rec(), _rec()]


def test_ties_of_a_group_by_code_then_position():
    L = 3
    words, census = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64)
    ev = OR.make_events([(2, (2, 2, 2), None), (0, (1, 0, 0), None), (0, (0, 0, 1), None), (2, (0, 0, 2), None)])
    assert OR.absorb(words, census, ev, 0, len(ev), L) == 1                     # one ordinal for all four
    state = (words != 0).astype(np.int64)
    labels = state.copy()                                                          # one grain holds all four
    layers, grains = OR.profile(words, state, labels, 1)
    # every voxel has ordinal 0: the depositions (code 1) come before the nucleations (code 2), the lower index first
    assert int(grains[0]["birth"]) == (1 << 24) | 1
    assert [int(x) for x in layers["birth"]] == [(1 << 24) | 1, (1 << 24) | 9, (2 << 24) | 26]
    assert _tuples(grains) == [_rec(4, (2, 2, 0, 0), 0, 0, 0, 0, 0, (1 << 24) | 1)]
    assert census[:, 0].tolist() == [1, 1, 0] and census[:, 2].tolist() == [1, 0, 1]


def test_identities():
    L = 3
    rs = np.random.RandomState(11)
    words, census = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64)
    rows = [(int(rs.randint(0, 4)), tuple(int(x) for x in rs.randint(0, L, 3)), tuple(int(x) for x in rs.randint(0, L, 3)))
            for _ in range(40)]
    OR.absorb(words, census, OR.make_events(rows), 0, 1, L)
    state = (rs.random_sample((L,) * 3) < 0.7).astype(np.int64)
    layers, _ = OR.profile(words, state)
    _, code = OR.decode(words)
    occ = state != 0
    assert [int(layers["n_by"][:, c - 1].sum()) for c in (1, 2, 3, 4)] == [int(np.count_nonzero(occ & (code == c))) for c in (1, 2, 3, 4)]
    assert np.array_equal(layers["n_occ"], layers["n_by"].sum(axis=1) + layers["n_unrec"])
    assert int(layers["n_occ"].sum()) == int(occ.sum())
    assert int(layers["n_left"].sum()) == int(np.count_nonzero(~occ & (code == 5)))
    assert int(census.sum()) == 40 + sum(1 for r in rows if r[0] == 1)          # a diffusion counts twice
    assert not layers["pad"].any()
