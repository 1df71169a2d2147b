"""cetkmc_thermal_cet / cetkmc_thermal_laser on an implicit handle with a thermal boundary (cetkmc_set_thermal_boundary,
DESIGN.md section 27) against the comparator tests/boundary_ref.update, bit for bit.

Inputs: tests/boundary_cases.py (implicit_cases' direct fields with the all-six boundary and the six single faces);
tests/test_boundary_ref_host.py checks on the comparator alone what they hold.  Sizes: boundary_cases.SIZES, the seams of
csrc/thermal_imp.hpp that the end addends meet (named there), and one case at 256; n = 1 and 3; both modes, two updates each.
Fields are compared as int64 views; where the comparator holds a NaN the engine must hold one; engine against engine every bit
is compared."""
import numpy as np
import pytest

import boundary_cases as bc
import boundary_ref as br
import implicit_cases as ic
from test_gpu_implicit_call import MS_KEYS, assert_same_field

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


def _engine(L, n, key, nonfinite=False):
    import cetkmc
    _, T0, prev, q = ic.direct_lattice(L, nonfinite)
    fields = ic.direct_fields(L)[0]
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    e.upload(fields[0], fields[1], fields[2], T0, fields[4])
    e.set_prev_state(prev)
    if n != 1:
        e.set_thermal_substeps(n)
    e.set_thermal_scheme("implicit")
    if key != "untouched":
        e.set_thermal_boundary(bc.BOUNDARIES[key])
    return e, q


def _update(e, mode, q):
    if mode == 1:
        e.thermal_cet(ic.DT, scrub_nan=True)
    else:
        e.thermal_laser(ic.DT, q, use_latent=True, scrub_nan=True)


def _info(updates, n, uploads=1):
    return dict(updates=updates, steps=updates * n, launches=3 * updates * n, coeff_uploads=uploads)


@pytest.mark.parametrize("mode", [1, 2], ids=["cet", "laser_latent"])
@pytest.mark.parametrize("n", bc.SUBSTEPS)
@pytest.mark.parametrize("L", bc.SIZES)
def test_all_six_faces_vs_comparator(oracle_mod, L, n, mode):
    """six different beta, T_ext inside, below and above the clip range; the infos after each call"""
    want, _ = bc.direct_reference(L, n, mode, "all")
    e, q = _engine(L, n, "all")
    try:
        for k in (1, 2):
            _update(e, mode, q)
            assert e.boundary_info() == _info(k, n)            # one [3][2][L] table for both updates
            assert e.implicit_info() == _info(k, n, uploads=0)  # every implicit update is counted; its own table was never built
        assert_same_field(e.download()["T"], want, f"L={L} n={n} mode={mode}")
        assert e.counters()["thermal_updates"] == 2
        got = e.thermal_boundary()
        assert all(np.array_equal(got[f], bc.ALL_SIX[f]) for f in ("beta", "T_ext", "ramp"))
    finally:
        e.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["cet", "laser_latent"])
@pytest.mark.parametrize("face", br.FACES)
def test_single_faces_vs_comparator(oracle_mod, face, mode):
    """L = 9, exactly one face active: a lo / hi or axis mix-up moves another face"""
    want, _ = bc.direct_reference(9, 1, mode, face)
    e, q = _engine(9, 1, face)
    try:
        for _ in range(2):
            _update(e, mode, q)
        assert_same_field(e.download()["T"], want, f"{face} mode={mode}")
        assert e.boundary_info() == _info(2, 1)
    finally:
        e.close()


def test_L256_vs_comparator(oracle_mod):
    L = 256
    want, _ = bc.direct_reference(L, 1, 2, "all", updates=1)
    e, q = _engine(L, 1, "all")
    try:
        _update(e, 2, q)
        assert_same_field(e.download()["T"], want, "L=256")
        assert e.boundary_info() == _info(1, 1)
    finally:
        e.close()


@pytest.mark.parametrize("L", [3, 9, 65])
def test_nonfinite_inputs_with_the_scrub(oracle_mod, L):
    """NaN, +inf and -inf on a face, an edge and a corner of a lattice with all six faces set (n = 3): step 1 removes them"""
    want, _ = bc.direct_reference(L, 3, 2, "all", nonfinite=True, updates=1)
    assert np.isfinite(want).all()
    e, q = _engine(L, 3, "all", nonfinite=True)
    try:
        _update(e, 2, q)
        assert_same_field(e.download()["T"], want, f"L={L}")
    finally:
        e.close()


def test_a_changed_beta_rebuilds_the_table_a_changed_T_ext_does_not(oracle_mod):
    L = 17
    lat, _, _, q = ic.direct_lattice(L)
    b0 = bc.ALL_SIX
    b1 = br.boundary(b0["beta"], b0["T_ext"] + 123.0, (5.0,) * 6)               # T_ext and ramp alone
    b2 = br.boundary(b0["beta"] * (1.0, 1.0, 1.0, 1.0, 1.0, 0.5), b1["T_ext"])   # one beta
    e, _ = _engine(L, 1, "all")
    try:
        for k, (b, uploads) in enumerate(((b0, 1), (b1, 1), (b2, 2), (b2, 2)), 1):
            e.set_thermal_boundary(b)
            br.update(lat, 1, ic.DT, 2, q, bc=b, u=0)
            _update(e, 2, q)
            assert_same_field(e.download()["T"], lat.T, f"update {k}")
            assert e.boundary_info() == _info(k, 1, uploads=uploads), k
        br.update(lat, 1, 0.5 * ic.DT, 2, q, bc=b2, u=0)                          # another dt: another r
        e.thermal_laser(0.5 * ic.DT, q, use_latent=True, scrub_nan=True)
        assert_same_field(e.download()["T"], lat.T, "changed dt")
        assert e.boundary_info() == _info(5, 1, uploads=3)
    finally:
        e.close()


@pytest.mark.parametrize("how", ["set_then_null", "all_beta_zero"])
@pytest.mark.parametrize("L", [9, 65])
def test_back_to_adiabatic_is_the_untouched_implicit_handle(L, how):
    """a boundary set and then set to NULL, and a boundary whose six beta are 0 (with T_ext and ramp set): every bit, counter and
    launch count of the implicit handle that never heard of a boundary"""
    out = []
    _, _, _, q = ic.direct_lattice(L)
    for key in ("untouched", how):
        e, _ = _engine(L, 1, "untouched")
        try:
            if key == "set_then_null":
                e.set_thermal_boundary(bc.ALL_SIX)
                e.set_thermal_boundary(None)
            elif key == "all_beta_zero":
                e.set_thermal_boundary(bc.BOUNDARIES["zero"])
            _update(e, 2, q)
            _update(e, 1, q)
            out.append((e.download(), {k: v for k, v in e.counters().items() if k not in MS_KEYS}, e.implicit_info(), e.boundary_info(), e.rate_sweep()))
        finally:
            e.close()
    (d0, c0, i0, b0, s0), (d1, c1, i1, b1, s1) = out
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert c0 == c1, {k: (c0[k], c1[k]) for k in c0 if c0[k] != c1[k]}
    assert i0 == i1 == _info(2, 1) and b0 == b1 == _info(0, 1, uploads=0) and s0 == s1
