"""Option early_tiles on the CPU: which launch stores a row, and that the apply block's rows do not depend on it.

A deferred step's selection launch runs the tiles [0, E) of the census-free tile range, the sweep launch behind it the tiles
[E, count); cetkmc_table_tile_of() is the one mapping of rows to tiles and cetkmc_early_tile_row() the side it puts a row on.
Here the mapping is restated (item = plane * ((L + 1) / 2) + row / 2, eight items per tile) and both exports are compared with
it for every row: each row has exactly one tile, every tile of the range owns rows, and early <=> tile < E.

The rows an event makes stale are stored by the apply block of the sweep launch, after both launches' tiles: its enumeration
(cetkmc_stale_rows) is a function of the record alone, so it names the same rows whichever side of E they lie on -- checked
against the predicate for every event type at corners, faces, plane L - 1, the interior and the rows around every seam."""
import ctypes as C

import pytest

SIZES = (129, 136, 160, 256)
EV_DEP, EV_DIFF, EV_NUC, EV_ATT = 0, 1, 2, 3


def _lib():
    from cetkmc import _lib
    _lib.build_library()
    return _lib.load()


def tile_count(L):
    return ((L + 1) // 2 * L + 7) // 8


def early_values(L):
    n = tile_count(L)
    return (0, 1, 8, 8 * (n // 16), n // 3, n - 1, n, n + 5)


def _pair(a):
    return (C.c_int * 2)(int(a[0]), int(a[1]))


def _stale_rows(lib, t, pos, tgt, L):
    rows = (C.c_int * 64)(*([-99] * 64))
    n = lib.cetkmc_stale_rows(t, _pair(pos), _pair(tgt), L, rows)
    assert 0 <= n <= 22
    return [(rows[2 * q], rows[2 * q + 1]) for q in range(n)]


@pytest.mark.parametrize("L", SIZES)
def test_rows_are_partitioned_into_early_and_late_tiles(L):
    lib = _lib()
    n, ipp = tile_count(L), (L + 1) // 2
    tile = [[lib.cetkmc_table_tile_of(L, gi, j) for j in range(L)] for gi in range(L)]
    owners = set()
    for gi in range(L):
        for j in range(L):
            assert tile[gi][j] == (gi * ipp + j // 2) // 8, (gi, j)        # one tile per row, the restated mapping
            owners.add(tile[gi][j])
    assert owners == set(range(n))                                         # the range has no tile without rows, none beyond it
    for E in early_values(L):
        n_early = 0
        for gi in range(L):
            for j in range(L):
                side = lib.cetkmc_early_tile_row(L, E, gi, j)
                assert side == (1 if tile[gi][j] < E else 0), (E, gi, j, side)
                n_early += side
        assert (n_early == 0) == (E == 0) and (n_early == L * L) == (E >= n), (E, n_early)
    for (gi, j) in ((-1, 0), (0, -1), (L, 0), (0, L)):
        assert lib.cetkmc_table_tile_of(L, gi, j) == -1 and lib.cetkmc_early_tile_row(L, 8, gi, j) == -1


def _seam_sites(lib, L, E):
    """sites whose 5 x 5 window of rows meets the seam between tile E - 1 and tile E: the first row of tile E and its neighbours"""
    ipp = (L + 1) // 2
    item = 8 * E
    gi, j = item // ipp, 2 * (item % ipp)
    if gi >= L:
        return []
    assert lib.cetkmc_table_tile_of(L, gi, j) == E and (E == 0 or lib.cetkmc_table_tile_of(L, gi, max(j - 1, 0)) in (E - 1, E))
    return [(min(max(gi + di, 0), L - 1), min(max(j + dj, 0), L - 1)) for di in (-1, 0, 1) for dj in (-2, -1, 0, 1)]


@pytest.mark.parametrize("L", SIZES)
def test_stale_rows_are_a_function_of_the_record_alone(L):
    lib = _lib()
    n = tile_count(L)
    sites = [(0, 0), (0, L - 1), (L - 1, 0), (L - 1, L - 1), (0, L // 2), (L // 2, 0), (L // 2, L - 1), (L - 1, L // 2), (L // 2, L // 3)]
    for E in (1, 8, 8 * (n // 16), n - 1):
        sites += _seam_sites(lib, L, E)
    both_sides = 0
    for (pi, pj) in sites:
        for t in (EV_DEP, EV_DIFF, EV_NUC, EV_ATT):
            targets = [(pi, pj)]
            if t == EV_DIFF:
                targets = [(pi + di, pj + dj) for di in (-1, 0, 1) for dj in (-1, 0, 1)
                           if (di or dj) and 0 <= pi + di < L and 0 <= pj + dj < L]
            for tgt in targets:
                rows = _stale_rows(lib, t, (pi, pj), tgt, L)
                assert len(set(rows)) == len(rows) and all(0 <= gi < L and 0 <= j < L for gi, j in rows), (t, pi, pj, tgt, rows)
                lo_i, hi_i = max(min(pi, tgt[0]) - 3, 0), min(max(pi, tgt[0]) + 4, L)
                lo_j, hi_j = max(min(pj, tgt[1]) - 3, 0), min(max(pj, tgt[1]) + 4, L)
                want = {(gi, j) for gi in range(lo_i, hi_i) for j in range(lo_j, hi_j)
                        if lib.cetkmc_stale_row(t, _pair((pi, pj)), _pair(tgt), gi, j)}
                assert set(rows) == want, (t, pi, pj, tgt)                 # every stale row, no other, whatever E is
                for E in (1, 8, 8 * (n // 16), n - 1):
                    sides = {lib.cetkmc_early_tile_row(L, E, gi, j) for gi, j in rows}
                    assert sides <= {0, 1}
                    both_sides += int(sides == {0, 1})
    assert both_sides >= 8, both_sides            # the seam sites do put an event's rows on both sides
