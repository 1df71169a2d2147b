"""The stale rows of a pending event: one predicate (stale_row() in csrc/kernels.hpp, exported as cetkmc_stale_row) and the
apply block's enumeration of them (stale_candidate(), exported as cetkmc_stale_rows), on the CPU.

A sweep launch that applies a deferred event has two readers of that definition.  The tiles that can hold such a row leave
its store out, by the predicate; the apply block stores every row its enumeration names, once, after the event.  A row
the predicate accepts and the enumeration misses is stored by nobody (it keeps the previous step's sums); a row the
enumeration names and the predicate rejects is stored twice, by a tile that may have read the lattice before the event.
Either shows on the GPU only by timing, so the two are compared here over every event type and site class, and the set
is checked against the rows whose sums the oracle changes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import PKG
from helpers import random_lattice

EV_DEP, EV_DIFF, EV_NUC, EV_ATT = 0, 1, 2, 3
# (di, dj) of the 14 neighbours of a voxel, the possible targets of a diffusion: same row (k +- 2), neighbours in i and j
# ((+-1, +-1, 0)), in j alone ((0, +-1, +-1), (0, +-2, 0)) and in i alone ((+-2, 0, 0))
NEIGHBOUR_ROWS = [(0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1), (0, 1), (0, -1), (0, 2), (0, -2), (2, 0), (-2, 0)]


def _lib():
    from cetkmc import _lib
    _lib.build_library()
    return _lib.load()


def _patch_max():
    src = open(os.path.join(PKG, "csrc", "kernels.hpp")).read()
    m = re.search(r"constexpr\s+int\s+PATCH_MAX\s*=\s*(\d+)\s*;", src)
    assert m, "PATCH_MAX not found in csrc/kernels.hpp"
    return int(m.group(1))


def _pair(a):
    return (C.c_int * 2)(int(a[0]), int(a[1]))


def _predicate(lib, t, pos, tgt, gi, j):
    return bool(lib.cetkmc_stale_row(t, _pair(pos), _pair(tgt), int(gi), int(j)))


def _enumeration(lib, t, pos, tgt, L):
    """the rows the apply block evaluates, in its order"""
    rows = (C.c_int * 64)(*([-99] * 64))
    n = lib.cetkmc_stale_rows(t, _pair(pos), _pair(tgt), L, rows)
    assert 0 <= n <= 32
    return [(rows[2 * q], rows[2 * q + 1]) for q in range(n)]


def _restated(lib, t, pos, tgt, L):
    """the double loop of the parent's apply block, from dirty_offset alone: each site's dirty offsets inside the lattice,
    the second site's without those that are rows of the first as well"""
    rule = lambda di, dj: bool(lib.cetkmc_dirty_offset(int(di), int(dj)))
    out = []
    if t < 0:
        return out
    for v in range(2 if t == EV_DIFF else 1):
        ci, cj = (tgt if v else pos)[:2]
        for di in range(-2, 3):
            for dj in range(-2, 3):
                gi, j = ci + di, cj + dj
                if not rule(di, dj) or not (0 <= gi < L and 0 <= j < L):
                    continue
                if v and rule(gi - pos[0], j - pos[1]):
                    continue
                out.append((gi, j))
    return out


def _predicate_set(lib, t, pos, tgt, L, full):
    """{(gi, j) in the lattice : predicate}: the whole lattice when `full`, else the 9 x 9 windows of both sites (the
    predicate is false further out: checked on random far rows by the caller)"""
    if full:
        cand = [(gi, j) for gi in range(L) for j in range(L)]
    else:
        cand = {(c[0] + di, c[1] + dj) for c in (pos, tgt) for di in range(-4, 5) for dj in range(-4, 5)}
        cand = [(gi, j) for gi, j in cand if 0 <= gi < L and 0 <= j < L]
    return {(gi, j) for gi, j in cand if _predicate(lib, t, pos, tgt, gi, j)}


def _sites(L, rs):
    e = L - 1
    corners = [(i, j) for i in (0, e) for j in (0, e)]
    faces = [(0, L // 2), (e, L // 2), (L // 2, 0), (L // 2, e), (1, 1), (e - 1, e - 1), (1, e), (e, 1)]
    seams = [(i, j) for i in (7, 8, 9, 15, 16) for j in (7, 8, 9, 16) if i < L and j < L]       # tile seams: multiples of 8
    rnd = [tuple(int(x) for x in rs.randint(0, L, 2)) for _ in range(12)]
    return corners + faces + seams + rnd


def _check_record(lib, t, pos, tgt, L, patch_max, full):
    enum = _enumeration(lib, t, pos, tgt, L)
    tag = (t, pos, tgt, L)
    assert len(enum) == len(set(enum)), (tag, "a row named twice", enum)
    assert len(enum) <= patch_max, (tag, len(enum))
    assert all(0 <= gi < L and 0 <= j < L for gi, j in enum), (tag, enum)
    pred = _predicate_set(lib, t, pos, tgt, L, full)
    assert pred == set(enum), (tag, "predicate only", sorted(pred - set(enum)), "enumeration only", sorted(set(enum) - pred))
    restated = _restated(lib, t, pos, tgt, L)
    assert sorted(restated) == sorted(enum), (tag, restated, enum)
    return enum


@pytest.mark.parametrize("L", [7, 10, 24, 129])
def test_predicate_equals_the_apply_blocks_enumeration(L):
    """Every event type, sites at corners, faces, tile seams and random places; diffusions to every neighbour row (same
    row, neighbours in i, in j, in both) and to far and coincident targets -- the predicate is a function of the record,
    whatever the record holds."""
    lib = _lib()
    patch_max = _patch_max()
    rs = np.random.RandomState(L)
    full = L <= 10
    n_rec, sizes = 0, set()
    for pos in _sites(L, rs):
        for t in (EV_DEP, EV_NUC, EV_ATT):
            # a one-site record ignores its target, whatever it holds
            for tgt in ((0, 0), (pos[0] + 1, pos[1] + 1)):
                enum = _check_record(lib, t, pos, tgt, L, patch_max, full)
                assert len(enum) <= patch_max // 2
                n_rec += 1
        targets = [(pos[0] + di, pos[1] + dj) for di, dj in NEIGHBOUR_ROWS]
        targets = [g for g in targets if 0 <= g[0] < L and 0 <= g[1] < L]
        targets += [tuple(int(x) for x in rs.randint(0, L, 2)), (L - 1 - pos[0], L - 1 - pos[1])]
        for tgt in targets:
            enum = _check_record(lib, EV_DIFF, pos, tgt, L, patch_max, full)
            sizes.add(len(enum))
            n_rec += 1
        # far from both sites the predicate is false (the tiles' window test relies on |d| <= 2)
        for _ in range(20):
            gi, j = (int(x) for x in rs.randint(-3, L + 3, 2))
            near = any(max(abs(gi - c[0]), abs(j - c[1])) <= 2 for c in (pos, targets[0]))
            if not near:
                assert not _predicate(lib, EV_DIFF, pos, targets[0], gi, j)
    assert n_rec >= 300
    if L >= 24:
        assert patch_max in sizes and 11 in sizes, sizes        # two disjoint interior sites; two sites of one row


def test_no_event_no_stale_rows():
    """type < 0 (a selection that terminated or ran out of stream): nothing is stale, whatever the sites hold"""
    lib = _lib()
    for t in (-1, -7):
        for pos, tgt in (((5, 5), (5, 6)), ((0, 0), (0, 0))):
            assert _enumeration(lib, t, pos, tgt, 16) == []
            assert not any(_predicate(lib, t, pos, tgt, gi, j) for gi in range(-1, 12) for j in range(-1, 12))


def test_interior_site_has_eleven_rows_and_the_window_bound():
    lib = _lib()
    enum = _enumeration(lib, EV_NUC, (20, 20), (0, 0), 64)
    assert len(enum) == 11 and (20, 20) in enum
    assert all(max(abs(gi - 20), abs(j - 20)) <= 2 for gi, j in enum)
    both = _enumeration(lib, EV_DIFF, (20, 20), (40, 40), 64)
    assert len(both) == 22 == _patch_max()


def _changed_rows(before, after):
    (s0, c0), (s1, c1) = before, after
    ch = (c0 != c1) | ~((s0 == s1) | (np.isnan(s0) & np.isnan(s1)))
    return {(int(i), int(j)) for i, _, j in np.argwhere(ch)}


@pytest.mark.parametrize("L,seed", [(7, 3), (10, 4)])
def test_stale_set_covers_the_oracles_changed_rows(oracle_mod, L, seed):
    """Make the change each event kind makes on the oracle -- an atom placed (deposition, nucleation, attachment: one site)
    or moved to a neighbour (diffusion: two sites) -- and compare the rows whose sums changed with the record's stale set."""
    lib = _lib()
    patch_max = _patch_max()
    rs = np.random.RandomState(200 + seed)
    state, theta, phi, T, defects = random_lattice(L, seed, fill=0.4)
    lat = oracle_mod.Lattice(state, theta, phi, T, defects, impurity_c=0.2)
    nb3 = [(1, 1, 0), (1, -1, 0), (-1, 1, 0), (-1, -1, 0), (0, 1, 1), (0, 1, -1), (0, -1, 1), (0, -1, -1),
           (2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2)]
    e = L - 1
    sites = [(i, j, k) for i in (0, e) for j in (0, e) for k in (0, e)] + [(0, L // 2, 1), (L // 2, e, 2), (e, 1, L // 2)]
    sites += [tuple(int(x) for x in rs.randint(0, L, 3)) for _ in range(12)]
    n_one = n_two = 0

    def get(p):
        return lat.state[p], lat.theta[p], lat.phi[p], lat.defects[p]

    def put(p, v):
        lat.state[p], lat.theta[p], lat.phi[p], lat.defects[p] = v

    for p in sites:
        old = get(p)
        base = tuple(a.copy() for a in lat.row_sums())
        for t, new_state in ((EV_DEP, 1), (EV_NUC, 1), (EV_ATT, 3), (EV_DEP, 2)):
            if new_state == old[0]:
                continue
            put(p, (new_state, rs.uniform(0, np.pi), rs.uniform(0, 2 * np.pi), 1 - old[3]))
            rows = _changed_rows(base, lat.row_sums())
            stale = set(_enumeration(lib, t, p[:2], (0, 0), L))
            assert rows <= stale and len(stale) <= patch_max // 2, (t, p, sorted(rows - stale))
            n_one += 1
            put(p, old)
        for d in nb3:
            q = (p[0] + d[0], p[1] + d[1], p[2] + d[2])
            if not all(0 <= x < L for x in q):
                continue
            oq = get(q)
            if old[0] == oq[0]:
                continue
            put(p, oq)                      # whatever sits at the two sites changes places
            put(q, old)
            rows = _changed_rows(base, lat.row_sums())
            stale = set(_enumeration(lib, EV_DIFF, p[:2], q[:2], L))
            assert rows <= stale and len(stale) <= patch_max, (p, q, sorted(rows - stale))
            assert stale == _predicate_set(lib, EV_DIFF, p[:2], q[:2], L, True)
            n_two += 1
            put(p, old)
            put(q, oq)
        assert not _changed_rows(base, lat.row_sums())
    assert n_one >= 40 and n_two >= 60, (n_one, n_two)
