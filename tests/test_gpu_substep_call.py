"""cetkmc_thermal_cet / cetkmc_thermal_laser on a handle with thermal_substeps = n against n oracle updates with dt / n
(tests/substep_ref.update), bit for bit.

Inputs: tests/substep_cases.direct_fields -- a rough field over the whole clip range, freshly filled voxels (latent heat), a
source with its peak on a lattice corner; tests/test_substep_ref_host.py checks on the comparator alone that they hold that.
Sizes and sub-step counts: substep_cases.SMALL_SIZES / LARGE_SIZES / SUBSTEPS and L = 256, chosen from the tile of
csrc/thermal_sub.hpp.  Fields are compared as int64 views; where the oracle holds a NaN the engine must hold a NaN (IEEE 754
leaves a NaN's sign and payload to the implementation: inf - inf is 0xFFF8... on x86 and 0x7FF8... on gfx950), engine against
engine every bit is compared."""
import numpy as np
import pytest

import substep_cases as sc

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_same_field(got, want, tag):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN positions", np.argwhere(np.isnan(got) != nan)[:4])
    bad = (_bits(got) != _bits(want)) & ~nan
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])


def _engine(L, n, options=None, nonfinite=False):
    import cetkmc
    fields, prev, q = sc.direct_fields(L)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    for k, v in ({} if options is None else options).items():
        e.set_option(k, v)
    T = sc.with_nonfinite(fields[3], L) if nonfinite else fields[3]
    e.upload(fields[0], fields[1], fields[2], T, fields[4])
    e.set_prev_state(prev)
    e.set_thermal_substeps(n)
    return e, q


def _update(e, mode, q, use_latent=True, scrub=True):
    if mode == 1:
        e.thermal_cet(1e-6, scrub_nan=scrub)
    else:
        e.thermal_laser(1e-6, q, use_latent=use_latent, scrub_nan=scrub)


def _expected_info(n, updates, S):
    if n == 1:
        return dict(updates=0, substeps=0, launches=0, blocked_launches=0)
    blocked = 0 if S == 1 else -(-(n - 1) // S)
    return dict(updates=updates, substeps=updates * n, launches=updates * (1 + (n - 1 if S == 1 else blocked)), blocked_launches=updates * blocked)


@pytest.mark.parametrize("mode", [1, 2], ids=["cet", "laser_latent"])
@pytest.mark.parametrize("n", sc.SUBSTEPS)
@pytest.mark.parametrize("L", sc.SMALL_SIZES)
def test_small_lattices_vs_oracle(oracle_mod, L, n, mode):
    """two updates (the second starts from a field with voxels on the clip values and, in laser mode, prev_state == state);
    the blocked kernel by option, plane groups of 8, so that L >= 9 has more than one"""
    want, _ = sc.direct_reference(L, n, mode, updates=2)
    e, q = _engine(L, n, dict(sc.BLOCKED, substep_planes=sc.PLANES))
    try:
        for _ in range(2):
            _update(e, mode, q)
        assert_same_field(e.download()["T"], want, f"L={L} n={n} mode={mode}")
        assert e.substep_info() == _expected_info(n, 2, sc.S_DEFAULT)
        assert e.counters()["thermal_updates"] == 2
    finally:
        e.close()


@pytest.mark.parametrize("mode,n", [(1, 17), (2, 5), (2, 17)], ids=["cet_n17", "laser_n5", "laser_n17"])
@pytest.mark.parametrize("L", sc.LARGE_SIZES)
def test_tile_columns_vs_oracle(oracle_mod, L, n, mode):
    """L = 121, 122, 123 (the tile's columns) and 129, default plane groups"""
    want, _ = sc.direct_reference(L, n, mode, threads=16)
    e, q = _engine(L, n, sc.BLOCKED)
    try:
        _update(e, mode, q)
        assert_same_field(e.download()["T"], want, f"L={L} n={n} mode={mode}")
        assert e.substep_info() == _expected_info(n, 1, sc.S_DEFAULT)
    finally:
        e.close()


def test_L256_fused_first_substep_vs_oracle(oracle_mod):
    """L = 256: sub-step 1 is the launch of the 16-row tiles that also write the rate table (of an intermediate field: the
    table is rewritten before the next sweep, which the stepping tests compare)"""
    L, n = 256, sc.S_DEFAULT + 2
    want, _ = sc.direct_reference(L, n, 2, threads=16)
    e, q = _engine(L, n)                                    # the default: S = 3
    try:
        _update(e, 2, q)
        assert_same_field(e.download()["T"], want, "L=256")
        assert e.substep_info() == _expected_info(n, 1, sc.S_DEFAULT)
        assert e.counters()["table_updates"] == 1           # sub-step 1 wrote it
    finally:
        e.close()


@pytest.mark.parametrize("scrub", [False, True], ids=["scrub_off", "scrub_on"])
@pytest.mark.parametrize("mode", [1, 2], ids=["cet", "laser_latent"])
@pytest.mark.parametrize("L", [5, sc.TJ + 1, sc.TK + 1])
def test_nonfinite_inputs_vs_oracle(oracle_mod, L, mode, scrub):
    """a NaN and a +inf on a face, an edge, a corner and the seam of the tile: with the scrub off the NaN spreads one cell
    per sub-step (n = 5: one launch of 3, one of 1), over seams and plane groups; with it on sub-step 1 removes both"""
    n = sc.S_DEFAULT + 2
    want, _ = sc.direct_reference(L, n, mode, scrub=scrub, nonfinite=True, threads=16 if L > 100 else 1)
    assert bool(np.isnan(want).any()) == (not scrub)
    e, q = _engine(L, n, dict(sc.BLOCKED, substep_planes=sc.PLANES), nonfinite=True)
    try:
        _update(e, mode, q, scrub=scrub)
        assert_same_field(e.download()["T"], want, f"L={L} mode={mode} scrub={scrub}")
    finally:
        e.close()


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("L", [sc.TJ + 1, 129])
def test_substep_block_option_is_bit_identical(L, S):
    """option substep_block = 1 (the plain path: n launches of the existing kernel), 2 and 4 against 3, every bit
    (non-finite voxels included, scrub off); blocked_launches says which kernel ran"""
    n, out = 17, []
    for opts in (sc.BLOCKED, {"substep_block": S}):
        e, q = _engine(L, n, opts, nonfinite=True)
        try:
            _update(e, 2, q, scrub=False)
            _update(e, 1, q, scrub=True)
            out.append((e.download()["T"], e.substep_info()))
        finally:
            e.close()
    (T0, i0), (T1, i1) = out
    assert np.array_equal(_bits(T0), _bits(T1)), np.argwhere(_bits(T0) != _bits(T1))[:4]
    assert i0 == _expected_info(n, 2, sc.S_DEFAULT) and i0["blocked_launches"] > 0
    assert i1 == _expected_info(n, 2, S) and (i1["blocked_launches"] == 0) == (S == 1)


@pytest.mark.parametrize("L", [sc.PLAIN_L, sc.PLAIN_L + 1])
def test_default_block_by_size(L):
    """without the option: the plain path up to L = 128 (measured faster there), k_thermal_sub with S = 3 above"""
    e, q = _engine(L, 17)
    try:
        _update(e, 2, q)
        assert e.substep_info() == _expected_info(17, 1, sc.default_block(L))
        assert (e.substep_info()["blocked_launches"] > 0) == (L > sc.PLAIN_L)
    finally:
        e.close()


def test_several_slabs_take_the_plain_path(oracle_mod):
    """three in-process slabs (two halo planes each way): n launches of the existing kernel, a halo exchange behind each"""
    import cetkmc
    L, n = 24, 5
    want, _ = sc.direct_reference(L, n, 2)
    fields, prev, q = sc.direct_fields(L)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, n_slabs=3)
    try:
        e.upload(*fields)
        e.set_prev_state(prev)
        e.set_thermal_substeps(n)
        _update(e, 2, q)
        assert_same_field(e.download()["T"], want, "three slabs")
        assert e.substep_info() == _expected_info(n, 1, 1)
    finally:
        e.close()
