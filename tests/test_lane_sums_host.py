"""lane_request() (csrc/kernels.hpp, exported as cetkmc_lane_request) against a restatement of its two conditions, on the CPU.

Under option lane_sums a lane of the census-free tiles holds its 8 class bytes and the count byte of its chunk and requests one
of three things: its 8 B lane sum (2) iff every class byte is 0x01 -- the voxel is empty and carries no event count, so
row_reduce() would let all 8 entries through the "empty" mask and nothing else -- and the count byte is a count (0..8, not the
poison 0xFF); else its 64 B of entries (1) iff cetkmc_lane_needs_values() holds; else nothing (0).  A lane sum must never be
chosen where row_reduce() would see a byte other than 0x01."""
import numpy as np
import pytest

NONE, VALUES, SUM = 0, 1, 2
PRISTINE = 0x0101010101010101
POISON = 0xFF


@pytest.fixture(scope="module")
def lib():
    from cetkmc import _lib
    _lib.build_library()
    return _lib.load()


def _bytes(w):
    return [(w >> (8 * h)) & 0xFF for h in range(8)]


def restated(w, cnt):
    b = _bytes(w)
    if all(x == 0x01 for x in b) and 0 <= cnt <= 8:
        return SUM
    if any((x & 1) or ((x & 2) and (x >> 2)) or (x & 0xFC) for x in b):       # row_reduce()'s two masks, or a stray count
        return VALUES
    return NONE


def _check(lib, w, cnt):
    got = lib.cetkmc_lane_request(int(w), int(cnt))
    assert got == restated(w, cnt), (hex(w), cnt, got)
    if got == SUM:
        assert all(x == 0x01 for x in _bytes(w)) and cnt != POISON, (hex(w), cnt)
    if got != SUM:      # without a usable lane sum the request is table_lane_skip's
        assert got == (VALUES if lib.cetkmc_lane_needs_values(int(w)) else NONE), (hex(w), cnt)


def test_header_names(lib):
    import re
    from conftest import ROOT
    src = open(f"{ROOT}/include/cetkmc.h").read()
    for name, v in (("NONE", NONE), ("VALUES", VALUES), ("SUM", SUM)):
        m = re.search(rf"\bCETKMC_LANE_REQ_{name}\s*=\s*(\d+)", src)
        assert m and int(m.group(1)) == v, name


def test_pristine_word_with_every_count_byte(lib):
    for cnt in range(256):
        want = SUM if cnt <= 8 else VALUES           # a poisoned (or meaningless) count: the entries, as before
        assert lib.cetkmc_lane_request(PRISTINE, cnt) == want == restated(PRISTINE, cnt), cnt
    assert lib.cetkmc_lane_request(PRISTINE, POISON) == VALUES


def test_named_cases(lib):
    cases = [
        (PRISTINE, 8, SUM), (PRISTINE, 0, SUM), (PRISTINE, POISON, VALUES),
        (0x0101010101010501, 8, VALUES), (0x0501010101010101, 0, VALUES),      # one listed empty voxel with a count
        (0x0101010A01010101, 7, VALUES), (0x0101010201010101, 7, VALUES),      # an atom with / without a count among empties
        (0x0202020202020202, 0, NONE), (0x0202020202020202, POISON, NONE),     # all solid, unexposed
        (0x0202020202020202, 8, NONE), (0x0000000000000000, 3, NONE),          # ... whatever the count byte says
        (0x0000000000000001, POISON, VALUES), (0x0000000000000001, 1, VALUES), # the padded last chunk of an odd L: k = L - 1, then outside
        (0x0000000000000002, 0, NONE), (0x0000000000000006, 0, VALUES),
    ]
    for w, cnt, want in cases:
        assert lib.cetkmc_lane_request(w, cnt) == want, (hex(w), cnt)
        _check(lib, w, cnt)


def test_one_byte_off_pristine(lib):
    """every byte value in every position of an otherwise pristine word, under a count and under the poison: a lane sum only for
    the pristine word itself"""
    for h in range(8):
        for b in range(256):
            w = (PRISTINE & ~(0xFF << (8 * h))) | (b << (8 * h))
            for cnt in (0, 5, 8, 9, POISON):
                _check(lib, w, cnt)
                if b != 0x01:
                    assert lib.cetkmc_lane_request(w, cnt) != SUM, (hex(w), cnt)


def test_random_words(lib):
    rs = np.random.RandomState(20261)
    kinds = np.array([0x00, 0x01, 0x02, 0x05, 0x0A, 0x09], np.uint8)
    rows = rs.choice(kinds, size=(40000, 8), p=[0.1, 0.6, 0.2, 0.04, 0.04, 0.02])
    rows[rs.random_sample(40000) < 0.3] = 0x01
    cnts = rs.choice(np.array([0, 1, 7, 8, 9, 200, POISON]), size=40000)
    for row, cnt in zip(rows, cnts):
        _check(lib, int.from_bytes(row.tobytes(), "little"), int(cnt))
    for w in rs.randint(0, 2 ** 63, 20000, dtype=np.int64):
        _check(lib, int(w), int(rs.randint(0, 256)))
