"""cetkmc_thermal_cet / cetkmc_thermal_laser on a handle with the implicit scheme against the comparator
(tests/implicit_ref.update), bit for bit.

Inputs: tests/implicit_cases.direct_fields -- a rough field over the whole clip range with planes below T_clip_lo, freshly
filled voxels (latent heat), a source with its peak on a lattice corner strong enough to reach T_clip_hi;
tests/test_implicit_ref_host.py checks on the comparator alone that they hold that.  Sizes: implicit_cases.SIZES (the
definition's sizes and the seams of csrc/thermal_imp.hpp, named there) and one case at 256; n = 1, 2, 3.  Fields are compared
as int64 views; where the comparator holds a NaN the engine must hold a NaN (IEEE 754 leaves a NaN's sign to the
implementation); engine against engine every bit is compared."""
import numpy as np
import pytest

import implicit_cases as ic

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1
MS_KEYS = ("ms_thermal", "ms_interface", "ms_sweep", "ms_dirty_rows", "ms_reduce", "ms_select_apply", "ms_comm")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same_field(got, want, tag):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN positions", np.argwhere(np.isnan(got) != nan)[:4])
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def _engine(L, n, nonfinite=False, only_nan=False, scheme="implicit"):
    import cetkmc
    _, T0, prev, q = ic.direct_lattice(L, nonfinite, only_nan)
    fields = ic.direct_fields(L)[0]
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    e.upload(fields[0], fields[1], fields[2], T0, fields[4])
    e.set_prev_state(prev)
    if n != 1:
        e.set_thermal_substeps(n)
    if scheme is not None:
        e.set_thermal_scheme(scheme)
    return e, q


def _update(e, mode, q, use_latent=True, scrub=True):
    if mode == 1:
        e.thermal_cet(ic.DT, scrub_nan=scrub)
    else:
        e.thermal_laser(ic.DT, q, use_latent=use_latent, scrub_nan=scrub)


def _info(updates, n, uploads=1):
    return dict(updates=updates, steps=updates * n, launches=3 * updates * n, coeff_uploads=uploads)


@pytest.mark.parametrize("mode", [1, 2], ids=["cet", "laser_latent"])
@pytest.mark.parametrize("n", ic.SUBSTEPS)
@pytest.mark.parametrize("L", ic.SIZES)
def test_sizes_vs_comparator(oracle_mod, L, n, mode):
    """two updates: the second starts from a field with voxels on the clip values and, in laser mode, prev_state == state"""
    want, _ = ic.direct_reference(L, n, mode, updates=2)
    e, q = _engine(L, n)
    try:
        for _ in range(2):
            _update(e, mode, q)
        d = e.download()
        assert_same_field(d["T"], want, f"L={L} n={n} mode={mode}")
        assert e.implicit_info() == _info(2, n)                 # one table for both updates: r did not change
        assert e.counters()["thermal_updates"] == 2
        assert e.substep_info() == dict(updates=0, substeps=0, launches=0, blocked_launches=0)
    finally:
        e.close()


def test_L256_vs_comparator(oracle_mod):
    L, n = 256, 2
    want, _ = ic.direct_reference(L, n, 2)
    e, q = _engine(L, n)
    try:
        _update(e, 2, q)
        assert_same_field(e.download()["T"], want, "L=256")
        assert e.implicit_info() == _info(1, n)
    finally:
        e.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["cet", "laser_latent"])
@pytest.mark.parametrize("L", [3, 5, 33, 65, 129])
def test_nonfinite_inputs_with_the_scrub(oracle_mod, L, mode):
    """NaN, +inf and -inf on a face, an edge, a corner and the chunk seam: step 1 removes them (n = 2)"""
    want, _ = ic.direct_reference(L, 2, mode, nonfinite=True)
    assert np.isfinite(want).all()
    e, q = _engine(L, 2, nonfinite=True)
    try:
        _update(e, mode, q)
        assert_same_field(e.download()["T"], want, f"L={L} mode={mode}")
    finally:
        e.close()


@pytest.mark.parametrize("L", [5, 65])
def test_one_nan_without_the_scrub(oracle_mod, L):
    """the solves carry it along every line: after the third the whole lattice is NaN, in the comparator and on the device"""
    want, _ = ic.direct_reference(L, 1, 1, scrub=False, only_nan=True)
    assert np.isnan(want).all()
    e, q = _engine(L, 1, only_nan=True)
    try:
        _update(e, 1, q, scrub=False)
        assert_same_field(e.download()["T"], want, f"L={L}")
    finally:
        e.close()


def test_laser_without_latent_heat_and_a_changed_dt(oracle_mod):
    """use_latent off; then a second update with another dt: the coefficient table is rebuilt once"""
    import implicit_ref
    L = 33
    lat, _, _, q = ic.direct_lattice(L)
    implicit_ref.update(lat, 1, ic.DT, 2, q, use_latent=False)
    implicit_ref.update(lat, 1, 0.5 * ic.DT, 2, q, use_latent=False)
    e, _ = _engine(L, 1)
    try:
        e.thermal_laser(ic.DT, q, use_latent=False, scrub_nan=True)
        e.thermal_laser(0.5 * ic.DT, q, use_latent=False, scrub_nan=True)
        assert_same_field(e.download()["T"], lat.T, "no latent heat")
        assert e.implicit_info() == _info(2, 1, uploads=2)
    finally:
        e.close()


@pytest.mark.parametrize("L", [33, 129])
def test_back_to_explicit_is_the_untouched_handle(L):
    """implicit update, scheme back to explicit, the same fields uploaded again: the next updates equal, in every bit and
    counter, those of a handle that made an explicit update where the other made the implicit one"""
    out = []
    fields, prev, q = ic.direct_fields(L)
    for scheme in ("implicit", None):
        e, _ = _engine(L, 1, scheme=scheme)
        try:
            _update(e, 2, q)
            if scheme:
                assert e.implicit_info()["updates"] == 1
                e.set_thermal_scheme("explicit")
            e.upload(*fields)
            e.set_prev_state(prev)
            c0 = e.counters()
            _update(e, 2, q)
            _update(e, 1, q)
            c1 = e.counters()
            out.append((e.download(), {k: c1[k] - c0[k] for k in c1 if k not in MS_KEYS}, e.implicit_info()["updates"], e.rate_sweep()))
        finally:
            e.close()
    (d0, c0, i0, s0), (d1, c1, i1, s1) = out
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert c0 == c1, {k: (c0[k], c1[k]) for k in c0 if c0[k] != c1[k]}
    assert (i0, i1) == (1, 0) and s0 == s1
