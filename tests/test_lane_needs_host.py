"""lane_needs_values() (csrc/kernels.hpp, exported as cetkmc_lane_needs_values) against a restatement of row_reduce()'s two uses
of a lane's rate-table entries, on the CPU.

The census-free tiles (option table_lane_skip) load a lane's 8 table entries only where the predicate holds for the lane's 8
class bytes.  row_reduce() uses entry h only behind two masks: ev[h] -- byte h has bit 0 (the voxel is empty) -- and dv[h] --
byte h has bit 1 (an atom) and a non-zero count in bits 7:2.  A lane the predicate rejects must be one whose entries no mask
lets through; the predicate is a superset of the masks (it also fires for a count on a byte with neither bit), and it is false
exactly for the words made of 0x00 and 0x02 bytes."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def needs():
    from cetkmc import _lib
    _lib.build_library()
    lib = _lib.load()
    return lambda w: bool(lib.cetkmc_lane_needs_values(int(w)))


def _bytes(w):
    return [(w >> (8 * h)) & 0xFF for h in range(8)]


def restated(w):
    """row_reduce(): the lane's values are used iff some byte is empty, or is an atom with a non-zero count"""
    return any((b & 1) or ((b & 2) and (b >> 2)) for b in _bytes(w))


def _check(needs, w):
    p = needs(w)
    assert p or not restated(w), hex(w)                                       # predicate false => no mask lets an entry through
    assert p == any(b not in (0x00, 0x02) for b in _bytes(w)), hex(w)         # true <=> some byte outside {0x00, 0x02}


def test_every_byte_value_in_every_position(needs):
    """each of the 256 byte values in each of the 8 positions, the other seven bytes all 0x00, all 0x02 or a mix of the two"""
    for rest in (0x0000000000000000, 0x0202020202020202, 0x0200020002000200, 0x0002000200020002):
        for h in range(8):
            for b in range(256):
                _check(needs, (rest & ~(0xFF << (8 * h))) | (b << (8 * h)))


def test_idle_words_are_false(needs):
    assert not needs(0x0000000000000000) and not needs(0x0202020202020202)
    for m in range(256):                                                      # every word of 0x00 / 0x02 bytes
        assert not needs(sum((0x02 if (m >> h) & 1 else 0x00) << (8 * h) for h in range(8)))


def test_random_words(needs):
    """1e5 seeded words: uniform ones (nearly all live) and words of mostly idle bytes with a few arbitrary ones"""
    rs = np.random.RandomState(20260)
    for w in rs.randint(0, 2 ** 63, 50000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, 50000).astype(np.uint64):
        _check(needs, int(w))
    idle = rs.choice(np.array([0x00, 0x02], np.uint8), size=(50000, 8))
    hit = rs.random_sample((50000, 8)) < 0.1
    idle[hit] = rs.randint(0, 256, int(hit.sum()))
    for row in idle:
        _check(needs, int.from_bytes(row.tobytes(), "little"))
