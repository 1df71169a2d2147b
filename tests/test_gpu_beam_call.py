"""cetkmc_thermal_beam on an implicit handle with a beam table (cetkmc_set_beam) against the comparator
tests/beam_ref.update, bit for bit.

Inputs: tests/beam_cases.py (implicit_cases' direct fields, a table of three rows from update ordinal 5: two beam positions and
an off row); tests/test_beam_ref_host.py checks on the comparator alone what they hold.  Sizes: beam_cases.SIZES and one case at
256; depth 1, 2 and L; n = 1 and 3; with and without latent heat; two consecutive ordinals each.  Fields are compared as int64
views; engine against engine every bit is compared."""
import pytest

import beam_cases as bm
import beam_ref
import boundary_cases as bcs
import implicit_cases as ic
import implicit_ref
from test_gpu_implicit_call import MS_KEYS, assert_same_field

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.1


def _engine(L, n, table, T0=None, key="none"):
    import cetkmc
    fields, prev, _ = ic.direct_fields(L)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C)
    e.upload(fields[0], fields[1], fields[2], fields[3] if T0 is None else T0, fields[4])
    e.set_prev_state(prev)
    if n != 1:
        e.set_thermal_substeps(n)
    e.set_thermal_scheme("implicit")
    if bcs.BOUNDARIES[key] is not None:
        e.set_thermal_boundary(bcs.BOUNDARIES[key])
    if table is not None:
        e.set_beam(table)
    return e


def _info(updates, n, uploads=1):
    return dict(updates=updates, steps=updates * n, launches=3 * updates * n, table_uploads=uploads)


@pytest.mark.parametrize("L,D,n,latent", bm.DIRECT)
def test_two_ordinals_vs_comparator(oracle_mod, L, D, n, latent):
    want, _ = bm.direct_reference(L, D, n, latent)
    e = _engine(L, n, bm.direct_table(L, D))
    try:
        for k, u in enumerate((bm.U0, bm.U0 + 1), 1):
            e.thermal_beam(bm.DT, u, use_latent=latent, scrub_nan=True)
            assert e.beam_info() == _info(k, n)
            assert e.implicit_info()["updates"] == k            # every implicit update is counted
        assert_same_field(e.download()["T"], want, f"L={L} D={D} n={n} latent={latent}")
        assert e.counters()["thermal_updates"] == 2
    finally:
        e.close()


def test_L256_vs_comparator(oracle_mod):
    L = 256
    want, _ = bm.direct_reference(L, 2, 1, True, ordinals=(bm.U0,))
    e = _engine(L, 1, bm.direct_table(L, 2))
    try:
        e.thermal_beam(bm.DT, bm.U0, use_latent=True, scrub_nan=True)
        assert_same_field(e.download()["T"], want, "L=256")
        assert e.beam_info() == _info(1, 1)
    finally:
        e.close()


@pytest.mark.parametrize("L,D", [(9, 2), (65, 2), (65, 65)])
def test_all_six_faces_vs_comparator(oracle_mod, L, D):
    """a section 27 boundary on all six faces: the beam stands between the ImpBc and nothing (n = 3)"""
    want, _ = bm.direct_reference(L, D, 3, True, key="all")
    e = _engine(L, 3, bm.direct_table(L, D), key="all")
    try:
        for u in (bm.U0, bm.U0 + 1):
            e.thermal_beam(bm.DT, u, use_latent=True, scrub_nan=True)
        assert_same_field(e.download()["T"], want, f"L={L} D={D}")
        assert e.beam_info() == _info(2, 3) and e.boundary_info()["updates"] == 2
    finally:
        e.close()


@pytest.mark.parametrize("L", [9, 65])
def test_nonfinite_values_inside_the_footprint_with_the_scrub(oracle_mod, L):
    want, _ = bm.nonfinite_reference(L, 2, 3)
    e = _engine(L, 3, bm.direct_table(L, 2), T0=bm.nonfinite_in_footprint(L, 2))
    try:
        e.thermal_beam(bm.DT, bm.U0, use_latent=True, scrub_nan=True)
        assert_same_field(e.download()["T"], want, f"L={L}")
    finally:
        e.close()


@pytest.mark.parametrize("L", [5, 64, 65])
def test_depth_one_equals_the_product_plane_through_thermal_laser(L):
    """D = 1: every bit of the same handle fed q = (amp * 1.0) * (gj x gk) through cetkmc_thermal_laser; and the off row equals
    the update from a plane of zeros"""
    t = bm.direct_table(L, 1)
    out = []
    for how in ("beam", "plane"):
        e = _engine(L, 1, t if how == "beam" else None)
        try:
            for x in (0, 1, 2):
                if how == "beam":
                    e.thermal_beam(bm.DT, bm.U0 + x, use_latent=True, scrub_nan=True)
                else:
                    e.thermal_laser(bm.DT, beam_ref.product_plane(t, x), use_latent=True, scrub_nan=True)
            out.append(e.download())
        finally:
            e.close()
    for f in out[0]:
        assert out[0][f].tobytes() == out[1][f].tobytes(), f


@pytest.mark.parametrize("L", [9, 65])
def test_set_then_null_is_the_untouched_implicit_handle(L):
    """a table set and removed again: every bit, counter and launch count of the implicit handle that never heard of a beam"""
    out = []
    _, _, _, q = ic.direct_lattice(L)
    for key in ("untouched", "set_then_null"):
        e = _engine(L, 1, None)
        try:
            if key == "set_then_null":
                e.set_beam(bm.direct_table(L, 2))
                e.set_beam(None)
            e.thermal_laser(bm.DT, q, use_latent=True, scrub_nan=True)
            e.thermal_cet(bm.DT, scrub_nan=True)
            info = e.beam_info()
            out.append((e.download(), {k: v for k, v in e.counters().items() if k not in MS_KEYS}, e.implicit_info(),
                        (info["updates"], info["steps"], info["launches"]), e.rate_sweep()))
        finally:
            e.close()
    (d0, c0, i0, b0, s0), (d1, c1, i1, b1, s1) = out
    for f in d0:
        assert d0[f].tobytes() == d1[f].tobytes(), f
    assert c0 == c1, {k: (c0[k], c1[k]) for k in c0 if c0[k] != c1[k]}
    assert i0 == i1 and b0 == b1 == (0, 0, 0) and s0 == s1


def test_a_new_table_replaces_the_old_and_diffusion_updates_ignore_it(oracle_mod):
    """two tables in turn on one handle (another depth); thermal_cet between them has no source"""
    L = 17
    lat, _, _, _ = ic.direct_lattice(L)
    ta, tb = bm.direct_table(L, 2), bm.direct_table(L, 17)
    e = _engine(L, 1, ta)
    try:
        e.thermal_beam(bm.DT, bm.U0, use_latent=True, scrub_nan=True)
        beam_ref.update(lat, 1, bm.DT, ta, bm.U0)
        e.thermal_cet(bm.DT, scrub_nan=True)
        implicit_ref.update(lat, 1, bm.DT, 1)
        e.set_beam(tb)
        e.thermal_beam(bm.DT, bm.U0 + 1, use_latent=True, scrub_nan=True)
        beam_ref.update(lat, 1, bm.DT, tb, bm.U0 + 1)
        assert_same_field(e.download()["T"], lat.T, "two tables")
        assert e.beam_info() == _info(2, 1, uploads=2) and e.implicit_info()["updates"] == 3
    finally:
        e.close()
