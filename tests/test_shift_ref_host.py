"""The comparator of cetkmc_shift (shift_ref.py) against hand-written cases and explicit loops, and what the inputs of the
GPU tests (shift_cases.py) claim to exercise -- asserted on the comparator alone.  No GPU."""
import numpy as np
import pytest

import shift_cases as SC
import shift_ref as SR


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _fields(L, seed):
    return SC.special_fields(L, seed)


def test_hand_written_2():
    st = np.arange(8).reshape(2, 2, 2) % 5
    f = dict(state=st, defects=(st == 3).astype(np.int64), theta=st * 0.5, phi=st * 0.25, T=1000.0 + st)
    out, info = SR.shift_fields(f, (1, 0, 0), fill_state=1, fill_T=7.0, fill_theta=0.5, fill_phi=0.75)
    assert out["state"].tolist() == [[[1, 1], [1, 1]], [[0, 1], [2, 3]]]
    assert out["defects"].tolist() == [[[0, 0], [0, 0]], [[0, 0], [0, 1]]]
    assert out["T"].tolist() == [[[7.0, 7.0], [7.0, 7.0]], [[1000.0, 1001.0], [1002.0, 1003.0]]]
    assert out["theta"][0].tolist() == [[0.5, 0.5], [0.5, 0.5]] and out["phi"][0, 0, 0] == 0.75
    assert info == dict(kept=4, exposed=4, dropped=[1, 1, 1, 0, 1, 0])      # old plane 1 held states 4, 0, 1, 2
    out, info = SR.shift_fields(f, (0, 0, -1), T_mode="edge")
    assert out["state"].tolist() == [[[1, 0], [3, 0]], [[0, 0], [2, 0]]]
    assert out["T"].tolist() == [[[1001.0, 1001.0], [1003.0, 1003.0]], [[1000.0, 1000.0], [1002.0, 1002.0]]]
    assert info == dict(kept=4, exposed=4, dropped=[1, 1, 1, 0, 1, 0])      # old k = 0 held states 0, 2, 4, 1
    out, info = SR.shift_fields(f, (0, -1, 1), fill_state=2)
    assert out["state"].tolist() == [[[2, 2], [2, 2]], [[2, 1], [2, 2]]]
    assert info["kept"] == 2 and info["exposed"] == 6


def test_hand_written_3():
    L = 3
    st = (np.arange(27).reshape(3, 3, 3) * 7) % 5
    T = np.arange(27, dtype=np.float64).reshape(3, 3, 3)
    f = dict(state=st, defects=np.zeros_like(st), theta=T * 0.0, phi=T * 0.0, T=T)
    out, info = SR.shift_fields(f, (1, -1, 2), fill_state=4, fill_T=-1.0)
    want_s = np.full((3, 3, 3), 4)
    want_T = np.full((3, 3, 3), -1.0)
    for i in range(L):
        for j in range(L):
            for k in range(L):
                s = (i - 1, j + 1, k - 2)
                if all(0 <= x < L for x in s):
                    want_s[i, j, k], want_T[i, j, k] = st[s], T[s]
    assert np.array_equal(out["state"], want_s) and np.array_equal(out["T"], want_T)
    assert info["kept"] == 2 * 2 * 1 and sum(info["dropped"]) == 27 - 4
    # other states count under [5]
    f5 = dict(f, state=np.where(st == 2, 9, st))
    _, info5 = SR.shift_fields(f5, (3, 0, 0))
    assert info5["dropped"][5] == int((st == 2).sum()) and info5["dropped"][2] == 0


@pytest.mark.parametrize("L", [1, 2, 5, 8])
def test_zero_is_identity_and_large_exposes_all(L):
    f = _fields(L, 3)
    out, info = SR.shift_fields(f, (0, 0, 0), fill_state=3, fill_T=1.0, T_mode="edge")
    for k in SR.FIELDS:
        a, b = out[k], f[k]
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k
    assert info == dict(kept=L ** 3, exposed=0, dropped=[0] * 6)
    for d in [(L, 0, 0), (0, -L, 0), (0, 0, L + 3), (1, -(L + 7), 0)]:
        out, info = SR.shift_fields(f, d, fill_state=1, fill_T=np.inf, fill_theta=-0.0, fill_phi=np.nan)
        assert (out["state"] == 1).all() and (out["defects"] == 0).all() and np.isposinf(out["T"]).all()
        assert (_bits(out["theta"]) == _bits(np.array(-0.0))[()]).all() and np.isnan(out["phi"]).all()
        assert info["kept"] == 0 and info["exposed"] == L ** 3
        assert info["dropped"] == [int((f["state"] == x).sum()) for x in range(5)] + [0]


@pytest.mark.parametrize("d", [(2, 0, 0), (-1, 3, 0), (0, -2, 5), (4, 4, -4), (7, 0, 1), (-9, 2, 2)])
def test_edge_against_clamp_loop(d):
    L = 6
    f = _fields(L, 11)
    out, _ = SR.shift_fields(f, d, T_mode="edge")
    for i in range(L):
        for j in range(L):
            for k in range(L):
                s = tuple(min(max(v - x, 0), L - 1) for v, x in zip((i, j, k), d))
                assert _bits(out["T"][i, j, k]) == _bits(f["T"][s]), (i, j, k)
    # everything but T does not depend on the mode
    out_v, _ = SR.shift_fields(f, d, T_mode="value")
    for k in ("state", "defects"):
        assert np.array_equal(out[k], out_v[k])
    ins = SR.inside_mask(L, d)
    assert np.array_equal(_bits(out["T"])[ins], _bits(out_v["T"])[ins])


def test_counts_add_up():
    rs = np.random.RandomState(0)
    for L in (1, 3, 7, 9):
        f = _fields(L, L)
        for _ in range(12):
            d = rs.randint(-L - 2, L + 3, 3)
            _, info = SR.shift_fields(f, d)
            assert sum(info["dropped"]) == info["exposed"] == L ** 3 - info["kept"], (L, d, info)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("a,b", [(1, 2), (-3, -1), (4, 9), (-2, -7)])
def test_two_shifts_equal_their_sum(axis, a, b):
    L = 7
    f = _fields(L, 5)
    kw = dict(fill_state=2, fill_T=123.0, fill_theta=0.25, fill_phi=-0.0)
    da, db, dab = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    da[axis], db[axis], dab[axis] = a, b, a + b
    one, _ = SR.shift_fields(f, da, **kw)
    two, _ = SR.shift_fields(one, db, **kw)
    both, _ = SR.shift_fields(f, dab, **kw)
    for k in SR.FIELDS:
        x, y = two[k], both[k]
        assert np.array_equal(_bits(x), _bits(y)) if x.dtype == np.float64 else np.array_equal(x, y), k


def test_maps_and_census():
    L = 4
    rs = np.random.RandomState(1)
    m = dict(stamp=rs.randint(-1, 50, (L, L, L)).astype(np.int64), T_s=rs.rand(L, L, L), g=rs.rand(L, L, L, 3) - 0.5, cool=rs.rand(L, L, L))
    d = (-1, 2, 0)
    out = SR.shift_solid(m, d)
    ins = SR.inside_mask(L, d)
    assert (out["stamp"][~ins] == -1).all() and (_bits(out["g"])[~ins] == 0).all() and (_bits(out["cool"])[~ins] == 0).all()
    assert np.array_equal(out["g"][0, 2, 1], m["g"][1, 0, 1]) and out["stamp"][2, 3, 3] == m["stamp"][3, 1, 3]
    w = rs.randint(0, 1 << 40, (L, L, L)).astype(np.uint64)
    ow = SR.shift_origin_words(w, d)
    assert ow.dtype == np.uint64 and (ow[~ins] == 0).all() and ow[0, 2, 0] == w[1, 0, 0]
    c = rs.randint(0, 9, (L, 5))
    assert SR.shift_census(c, d).tolist() == c[1:].tolist() + [[0] * 5]
    assert SR.shift_census(c, (2, 5, 5)).tolist() == [[0] * 5] * 2 + c[:2].tolist()
    assert SR.shift_census(c, (0, 1, 1)).tolist() == c.tolist()
    assert not SR.shift_census(c, (-L, 0, 0)).any()


# ---- what the inputs of the GPU tests exercise ------------------------------------------------------------------------------
def test_special_fields_hold_the_special_values():
    for L in SC.CALL_SIZES:
        if L > 33:
            continue
        f = _fields(L, L)
        for k in ("T", "theta", "phi"):
            b = _bits(f[k])
            if L >= 3:
                assert (b == SC.NAN_PAYLOAD_BITS).any() and np.isposinf(f[k]).any() and np.isneginf(f[k]).any(), (L, k)
                assert (b == _bits(np.array(-0.0))[()]).any(), (L, k)
        assert set(np.unique(f["state"])) <= {0, 1, 2, 3, 4} and set(np.unique(f["defects"])) <= {0, 1}


def test_call_cases_cover_the_issue():
    for L in SC.CALL_SIZES:
        ds = SC.call_shifts(L)
        for a in range(3):
            for m in (1, 7, 8, 9, L - 1, L, L + 3):
                for sgn in ((1, -1) if m != L + 3 else (1,)):
                    if m == 0:
                        continue
                    d = [0, 0, 0]
                    d[a] = sgn * m
                    assert tuple(d) in ds, (L, d)
        for d in [(3, -5, 9), (-2, 0, 1), (0, 8, -8)]:
            assert d in ds
        assert (0, 0, 0) not in ds
    assert SC.CALL_SIZES == (1, 2, 3, 7, 8, 9, 33, 64, 65, 129, 136, 264)
    # a move along k that is no multiple of 8 reads the byte rows misaligned; at L > 8 a kept run straddles a lane
    f = _fields(9, 9)
    out, info = SR.shift_fields(f, (0, 0, -5))
    assert info["kept"] == 9 * 9 * 4 and np.array_equal(out["state"][:, :, :4], f["state"][:, :, 5:])
