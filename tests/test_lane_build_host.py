"""The chunk node as the temperature tiles form it (option lane_build), on the CPU.

k_thermal_tiles16<.., LANES> holds the 8 rate-table entries of a chunk in four consecutive lanes, two per lane.  Each lane adds
its pair, then the pair sum of its quad_perm partner (lane ^ 1), then the quad sum of the other pair of lanes (lane ^ 2).  The
row reduction enters the same 8 entries as tree8() = ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)); a lane sum that differs from it in the
last bit changes a row sum.  cetkmc_lane_quad_node restates the lanes' order (lane_quad_node() in csrc/kernels.hpp, the function
the kernel's comment points to), cetkmc_tree8 the row reduction's expression; both are compared bit for bit with a restatement
in numpy float64 arithmetic, in every lane, and the count with the number of non-zero entries."""
import ctypes as C

import numpy as np


def _lib():
    from cetkmc import _lib
    _lib.build_library()
    return _lib.load()


def _tree8_np(x):
    x = [np.float64(v) for v in x]
    return ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]))


def _quad_np(x, lane):
    """pairs, then quads, in the order lane `lane` adds: own operand first"""
    x = [np.float64(v) for v in x]
    p = [x[2 * a] + x[2 * a + 1] for a in range(4)]
    q = [p[a] + p[a ^ 1] for a in range(4)]
    return q[lane] + q[lane ^ 2]


def _chunks():
    rs = np.random.RandomState(11)
    tiny = np.float64(5e-324)
    out = [np.zeros(8), np.full(8, tiny), np.full(8, 2.2250738585072014e-308), np.full(8, 1.7e308 / 8)]
    for _ in range(4000):
        kind = rs.randint(5)
        if kind == 0:       # rates of one magnitude, as a row of the bulk table holds them
            x = rs.uniform(1.0, 2.0, 8) * 10.0 ** rs.randint(-30, 14)
        elif kind == 1:     # mixed magnitudes: every addition rounds
            x = rs.uniform(1.0, 2.0, 8) * 10.0 ** rs.randint(-300, 300, 8).clip(-300, 290)
        elif kind == 2:     # denormals beside normal numbers
            x = rs.randint(1, 1 << 20, 8).astype(np.float64) * tiny
            x[rs.randint(8)] = rs.uniform(1e-310, 1e-300)
        elif kind == 3:     # cancellation-free sums that differ by association: 1, ulp-sized and half-ulp-sized terms
            x = np.where(rs.random_sample(8) < 0.4, 1.0, rs.choice([2.0 ** -53, 2.0 ** -52, 3 * 2.0 ** -54], 8))
        else:
            x = rs.uniform(0.0, 1e13, 8)
        x[rs.random_sample(8) < 0.3] = 0.0          # entries without a rate are +0.0
        out.append(x)
    return out


def test_quad_node_is_tree8_in_every_lane():
    lib = _lib()
    differs_from_left_fold = 0
    for x in _chunks():
        buf = (C.c_double * 8)(*x)
        want = _tree8_np(x)
        t8 = np.float64(lib.cetkmc_tree8(buf))
        assert t8.tobytes() == want.tobytes(), (x, t8, want)
        for lane in range(4):
            s, n = C.c_double(), C.c_int()
            lib.cetkmc_lane_quad_node(buf, lane, C.byref(s), C.byref(n))
            got = np.float64(s.value)
            assert got.tobytes() == _quad_np(x, lane).tobytes(), (x, lane, got)
            assert got.tobytes() == want.tobytes(), ("lane node differs from tree8", x, lane, got, want)
            assert n.value == int(np.count_nonzero(x)), (x, lane, n.value)
        fold = np.float64(0.0)
        for v in x:
            fold = fold + np.float64(v)
        differs_from_left_fold += fold.tobytes() != want.tobytes()
    # the inputs tell an association order from another: a left fold of the same entries differs in many of them
    assert differs_from_left_fold > 500, differs_from_left_fold
