"""cetkmc_origin_absorb_events on the device against the comparator (origin_ref.py), ==: crafted records at L = 1 .. 129 --
every face, edge and corner with all three filling types, a diffusion along each of the 14 stencil offsets, skipped records,
a call of one record, 4096 records on three voxels (the maximum under contention), calls that follow each other (seq carries
on), group = 1, 7 and n -- and every refusal, which leaves the map as it was."""
import itertools

import numpy as np
import pytest

import origin_ref as OR

pytestmark = pytest.mark.gpu

STENCIL = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)] + list(itertools.product((1, -1), repeat=3))
assert len(STENCIL) == 14


def _crafted(L):
    """records over every face, edge and corner (coordinates 0, L // 2, L - 1), the three filling types in turn, then a
    diffusion along each stencil offset that fits, then records that are skipped"""
    rows = []
    coords = sorted({0, L // 2, L - 1})
    for q, pos in enumerate(itertools.product(coords, repeat=3)):
        rows.append(((0, 2, 3)[q % 3], pos, (0, 0, 0) if q % 3 == 2 else None))
    for d in STENCIL:
        pos = tuple(0 if x >= 0 else L - 1 for x in d)
        tgt = tuple(p + x for p, x in zip(pos, d))
        if all(0 <= t < L for t in tgt):
            rows.append((1, pos, tgt))
    rows += [(-1, (0, 0, 0), None), (-2, (L - 1,) * 3, None), (1, (0, 0, 0), (-1, -1, -1)), (-1, (-1, -1, -1), None), (7, (0, 0, 0), None)]
    return OR.make_events(rows)


def _contended(L, n=4096, seed=1):
    """n records on (at most) three voxels: fills of all types and diffusions between them"""
    rs = np.random.RandomState(seed)
    vox = [(0, 0, 0), (L - 1, L - 1, L - 1), (0, L - 1, 0)]
    rows = []
    for _ in range(n):
        t = int(rs.randint(0, 4))
        a, b = (vox[int(x)] for x in rs.randint(0, 3, 2))
        rows.append((t, a, b if t in (1, 3) else None))
    return OR.make_events(rows)


def _same(e, words, census, seq, tag):
    assert np.array_equal(e.origin_words(), words), tag
    assert np.array_equal(e.origin_census(), census), tag
    assert e.origin_seq() == seq, tag


@pytest.mark.parametrize("L", [1, 2, 3, 5, 33, 65, 129])
def test_absorb_vs_ref(L):
    import cetkmc
    e = cetkmc.Engine(L)
    try:
        assert e.origin_seq() == -1
        with pytest.raises(RuntimeError, match="needs a map"):
            e.origin_absorb(_crafted(L))
        with pytest.raises(RuntimeError, match="needs a map"):
            e.origin_words()
        e.origin_begin()
        words, census, seq = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64), 0
        _same(e, words, census, 0, "begin")
        crafted = _crafted(L)
        pad7 = OR.make_events([(-1, (0, 0, 0), None)] * (-len(crafted) % 7))
        calls = [(crafted[::-1], 1), (crafted[:1], 1), (np.concatenate([crafted, pad7]), 7), (crafted, len(crafted)),
                 (_contended(L), 1), (_contended(L, seed=2), 4096), (_contended(L, 4095, seed=3), 7), (crafted, 1)]
        for c, (ev, group) in enumerate(calls):
            e.origin_absorb(ev, group)
            seq = OR.absorb(words, census, ev, seq, group, L)
            _same(e, words, census, seq, f"L={L} call {c}")
        e.origin_absorb(crafted[:0], 3)                        # no record: nothing happens
        _same(e, words, census, seq, "n = 0")
        o, code = OR.decode(words)
        assert census.sum() > 0 and (L < 3 or set(np.unique(code)) >= {1, 2, 3, 4, 5})      # every code is in the final map
        # refusals: the map stays as it is
        bad_pos = OR.make_events([(0, (0, 0, 0), None), (2, (0, L, 0), None)])
        bad_tgt = OR.make_events([(1, (0, 0, 0), (0, 0, L))])
        bad_neg = OR.make_events([(3, (0, -1, 0), (0, 0, 0))])
        for ev, group, msg in ((crafted[:4], 0, "group"), (crafted[:4], -1, "group"), (crafted[:4], 3, "multiple"),
                               (bad_pos, 1, "position outside"), (bad_tgt, 1, "target outside"), (bad_neg, 1, "position outside")):
            with pytest.raises(RuntimeError, match=msg):
                e.origin_absorb(ev, group)
        assert e.lib.cetkmc_origin_absorb_events(e.h, None, 2, 1) != 0 and e.lib.cetkmc_origin_read(e.h, None) != 0
        assert e.lib.cetkmc_origin_census(e.h, None) != 0 and e.lib.cetkmc_origin_profile(e.h, None, 0, None) != 0
        _same(e, words, census, seq, "after the refusals")
        # a second begin resets map, census and clock; end frees the map
        e.origin_begin()
        _same(e, np.zeros_like(words), np.zeros_like(census), 0, "second begin")
        e.origin_end()
        assert e.origin_seq() == -1
        with pytest.raises(RuntimeError, match="needs a map"):
            e.origin_end()
    finally:
        e.close()


def test_apply_uses_one_ordinal():
    """cetkmc_apply absorbs its event: a select / apply loop against the comparator fed with the applied events"""
    import cetkmc
    from helpers import random_lattice
    L = 8
    e = cetkmc.Engine(L, impurity_c=0.2)
    try:
        e.upload(*random_lattice(L, 4))
        e.origin_begin()
        words, census, seq = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64), 0
        kinds = set()
        rs = np.random.RandomState(0)
        for s in range(40):
            total, n_events, _ = e.rate_sweep()
            ev = e.select(rs.random_sample() * total)
            if ev.type == 0:
                ev.atom = 1                                     # the species draw of a deposition is the caller's
            e.apply(ev, 0.3, 0.4, False)
            rec = OR.make_events([(ev.type, tuple(ev.pos), tuple(ev.target))])
            seq = OR.absorb(words, census, rec, seq, 1, L)
            kinds.add(int(ev.type))
        _same(e, words, census, 40, "select / apply loop")
        assert len(kinds) >= 2, kinds
        st = e.download()["state"]
        o, code = OR.decode(words)
        assert np.all(st[(code >= 1) & (code <= 4)] != 0) and np.all(st[code == 5] == 0)
    finally:
        e.close()
