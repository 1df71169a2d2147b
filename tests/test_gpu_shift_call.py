"""cetkmc_shift against the comparator tests/shift_ref.py: the five fields after one shift, bit for bit.

Sizes 1, 2, 3, 7, 8, 9, 33, 64, 65 (the lane tail, the row pitch), 129, 136 (half-wave rows, the pitch past 128) and 264
(full-wave rows); every d of shift_cases.call_shifts: each axis alone by +-1, +-7, +-8, +-9, +-(L - 1), +-L and L + 3 and the
mixed shifts (3, -5, 9), (-2, 0, 1), (0, 8, -8); both T modes; fill_state 0 and 1; NaN with a payload, a negative NaN, +-inf and
-0.0 in T, theta and phi of the lattice and among the fills.  The full cross of L, d, T mode and fill_state runs.  A
parametrised case is one (L, T mode, fill_state, group of d) and walks through its shifts on one handle; up to L = 136 the
group is every d, at L = 264, where a download and its comparison take half a second, the d of one axis or the mixed ones.

Where the previous shift left most of the lattice in place the next one starts from what it left (the comparator is fed
the fields the previous comparison proved the device holds); behind a shift by L - 1 or more the original is uploaded again.

Every shift also checks the info counts and that bytes_h2d + bytes_d2h grew by at most 256.  The sweep of the shifted
lattice (cetkmc_rate_sweep, cetkmc_row_sums) equals the oracle's on the comparator's fields after every shift up to L = 65,
after every sixth and behind the case's last shift above; cetkmc_enumerate_events equals the oracle's list after every shift at
L <= 9 and behind the last shift of every case up to L = 136.  At L = 264 the list (some 10^8 records of 64 bytes on either
side) is compared in one case, behind (-2, 0, 1).  d = 0 changes no byte and no cache:
cetkmc_row_sums is still served behind a warm sweep, and the counters do not move."""
import numpy as np
import pytest

import shift_cases as SC
import shift_ref as SR
from helpers import assert_fields_match_oracle, relerr
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1
SPECIALS = np.array([SC.NAN_PAYLOAD_BITS, SC.NEG_NAN_BITS], np.int64).view(np.float64).tolist() + [np.inf, -np.inf, -0.0]
FILL_T = [300.0, 3500.0] + SPECIALS
FILL_THETA = [0.0, 1.25, -0.0, SPECIALS[0], 3.0]
FILL_PHI = [0.5, 0.0, SPECIALS[1], 6.0, -0.0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, tag):
    for k in ("state", "defects"):
        assert np.array_equal(got[k], want[k]), (tag, k, np.argwhere(np.asarray(got[k]) != np.asarray(want[k]))[:4])
    for k in ("theta", "phi", "T"):
        g, w = _bits(got[k]), _bits(want[k])
        assert np.array_equal(g, w), (tag, k, np.argwhere(g != w)[:4])


def _download(e):
    return e.download_planes(0, e.L, state=True, theta=True, phi=True, T=True, defects=True)


def _upload(e, f):
    e.upload(f["state"], f["theta"], f["phi"], f["T"], f["defects"])


def _oracle(oracle_mod, f):
    return oracle_mod.Lattice(np.asarray(f["state"], np.int64), f["theta"], f["phi"], f["T"], np.asarray(f["defects"], np.int64),
                              impurity_c=IMPURITY_C)


def _events_match(e, lat, tag):
    ev_o, _ = lat.enumerate()
    ev_g, n_g = e.enumerate_events()
    assert n_g == len(ev_o), tag
    for f in ("type", "pos", "target", "atom"):
        assert np.array_equal(ev_g[f], ev_o[f]), (tag, f)
    if len(ev_o):
        assert relerr(ev_g["rate"], ev_o["rate"]).max() <= RATE_RTOL, tag


def _moved_bytes(e):
    c = e.counters()
    return c["bytes_h2d"] + c["bytes_d2h"]


GROUPS = ("axis0", "axis1", "axis2", "mixed")


def _cases():
    out = []
    for L in SC.CALL_SIZES:
        for T_mode in ("value", "edge"):
            for fill_state in (0, 1):
                out += [(L, T_mode, fill_state, g) for g in (GROUPS if L > 136 else ("all",))]
    return out


def _shifts_of(L, group):
    ds = SC.call_shifts(L)
    if group == "all":
        return ds
    if group == "mixed":
        return [d for d in ds if d in SC.MIXED]
    a = GROUPS.index(group)
    return [d for d in ds if d not in SC.MIXED and d[a] != 0]


@pytest.mark.parametrize("L,T_mode,fill_state,group", _cases())
def test_shift_vs_comparator(oracle_mod, L, T_mode, fill_state, group):
    import cetkmc
    oracle_mod.set_threads(16 if L > 100 else 1)
    orig = SC.special_fields(L, 100 + L)
    shifts = _shifts_of(L, group)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        cur, calls = None, 0
        for q, d in enumerate(shifts):
            tag = f"L={L} d={d} {T_mode} fill_state={fill_state}"
            last = q == len(shifts) - 1
            if cur is None:
                _upload(e, orig)
                cur = orig
            kw = dict(fill_state=fill_state, fill_T=FILL_T[q % len(FILL_T)], T_mode=T_mode, fill_theta=FILL_THETA[q % 5],
                      fill_phi=FILL_PHI[q % 5])
            b0 = _moved_bytes(e)
            info = e.shift(d, **kw)
            grew = _moved_bytes(e) - b0
            assert 0 <= grew <= 256, (tag, grew)
            calls += 1
            want, winfo = SR.shift_fields(cur, d, **kw)
            assert info == dict(winfo, calls=calls), (tag, info, winfo)
            _same(_download(e), want, tag)
            if L <= 65 or q % 6 == 0 or last:
                lat = _oracle(oracle_mod, want)
                assert_fields_match_oracle(e, lat, RATE_RTOL, tag)
                if L <= 9 or (last and L <= 136) or (L > 136 and d == (-2, 0, 1) and (T_mode, fill_state) == ("value", 0)):
                    _events_match(e, lat, tag)
            cur = want if max(abs(x) for x in d) < L - 1 and L > 9 else None
    finally:
        e.close()
        oracle_mod.set_threads(1)


@pytest.mark.parametrize("L", [1, 9, 65, 136])
def test_zero_shift_is_a_no_op(L):
    import cetkmc
    f = SC.physical_fields(L, 7)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    try:
        _upload(e, f)
        assert e.shift((1 if L > 1 else 2, 0, 0))["calls"] == 1
        before = _download(e)
        sweep = e.rate_sweep()
        rsum, rcnt = e.row_sums()
        c0 = e.counters()
        info = e.shift((0, 0, 0), fill_state=3, fill_T=np.nan, T_mode="edge", fill_theta=1.0, fill_phi=2.0)
        assert info == dict(calls=1, kept=L ** 3, exposed=0, dropped=[0] * 6)
        assert e.counters() == c0                      # nothing moved, nothing launched that the handle counts
        rsum1, rcnt1 = e.row_sums()                    # still served: the sweep cache is not stale
        assert np.array_equal(_bits(rsum), _bits(rsum1)) and np.array_equal(rcnt, rcnt1)
        _same(_download(e), before, f"L={L} d=0")
        assert e.rate_sweep() == sweep
    finally:
        e.close()
