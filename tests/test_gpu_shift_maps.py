"""The two maps move with the lattice (cetkmc_shift).

Maps with real records -- a solidification map and an origin map filled by Mode A stepping -- are shifted; afterwards
cetkmc_solid_read, cetkmc_origin_read and cetkmc_origin_census equal the comparator (shift_ref.py) applied to what they returned
before, the origin clock is unchanged, a cetkmc_solid_update right behind the shift reports nothing new and nothing cleared,
stepping on records the true transitions only (solid_ref.SolidRef from the shifted map and fields), and the profiles after a
re-clustering equal the NumPy comparators (solid_ref, origin_ref) on the shifted arrays."""
import numpy as np
import pytest

import origin_ref as OR
import shift_ref as SR
import solid_ref as SOL
from helpers import FOUR_KIND_PARAMS, batch_calls, random_lattice

pytestmark = pytest.mark.gpu

IMPURITY_C = 0.2
DT = 1e-6
ORIGIN_FIELDS = ("n_occ", "n_by", "n_unrec", "n_left", "ord_sum", "ord_min", "ord_max", "birth")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _engine(L, seed):
    import cetkmc
    params = cetkmc.default_params(IMPURITY_C)
    for k, v in FOUR_KIND_PARAMS.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=IMPURITY_C, params=params)
    e.upload(*random_lattice(L, seed))
    return e


def _step(e, calls):
    for step0, n, u_pick, u_def, u_np in calls:
        r = e.run_steps(step0, n, 0.05, u_pick, u_def, u_np, rng_mode=1, seed=9, thermal_mode=1)
        assert (r["done"], r["status"]) == (n, 0)


def _same_solid(got, want, tag):
    assert np.array_equal(got["stamp"], want["stamp"]) and got["stamp"].dtype == np.int64, tag
    for k in ("T_s", "g", "cool"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), (tag, k)


@pytest.mark.parametrize("L,d", [(16, (-3, 0, 0)), (16, (2, -1, 4)), (13, (0, 5, -8)), (13, (1, 0, 0)), (16, (-16, 0, 0))])
def test_maps_move_with_the_lattice(L, d):
    import cetkmc
    import constants
    e = _engine(L, 31 + L)
    try:
        e.solid_begin()
        e.origin_begin()
        calls = batch_calls((40, 40, 40, 40))
        for q in range(2):
            _step(e, calls[q:q + 1])
            e.solid_update(q + 1, DT)
        m0, w0, c0, seq0 = e.solid_read(), e.origin_words(), e.origin_census(), e.origin_seq()
        f0 = e.download(defects=True)
        assert (m0["stamp"] >= 0).sum() > 10 and (w0 != 0).sum() > 20 and seq0 == 80 and c0.sum() > 0
        assert set(np.unique(m0["stamp"])) >= {-1, 1, 2}

        b0 = e.counters()
        info = e.shift(d, fill_state=0, fill_T=3000.0)
        b1 = e.counters()
        assert (b1["bytes_h2d"] + b1["bytes_d2h"]) - (b0["bytes_h2d"] + b0["bytes_d2h"]) <= 256
        f1, winfo = SR.shift_fields(f0, d, fill_state=0, fill_T=3000.0)
        assert info == dict(winfo, calls=1)
        m1 = SR.shift_solid(m0, d)
        _same_solid(e.solid_read(), m1, "after the shift")
        assert np.array_equal(e.origin_words(), SR.shift_origin_words(w0, d))
        assert np.array_equal(e.origin_census(), SR.shift_census(c0, d))
        assert e.origin_seq() == seq0
        if max(abs(x) for x in d) < L:
            assert (m1["stamp"] >= 0).any() and 0 < (SR.shift_origin_words(w0, d) != 0).sum() < (w0 != 0).sum() + 1

        # the snapshot is the new state and T: nothing solidified, nothing cleared
        up = e.solid_update(3, DT)
        assert up == dict(n_new=0, n_cleared=0, n_recorded=int((m1["stamp"] >= 0).sum())), up
        _same_solid(e.solid_read(), m1, "after the empty update")

        # profiles of the shifted maps after a re-clustering
        scales = cetkmc.engine.default_solid_scales()
        ref = SOL.SolidRef.from_map(m1)
        cl = e.clusters(0.5, labels=True)
        assert np.array_equal(e.download()["state"], f1["state"])
        assert ref.ties(scales) == 0          # (of the input: no quantised value sits on a rounding boundary)
        got = e.solid_profile(scales, grains=True, recluster=False)
        want = ref.profile(scales, cl["labels"])
        assert SOL.same_records(got["layers"], want["layers"]) == [] and SOL.same_records(got["grains"], want["grains"]) == []
        lay, gr = OR.profile(SR.shift_origin_words(w0, d), f1["state"], cl["labels"], len(cl["size"]))
        got = e.origin_profile(grains=True, recluster=False)
        assert [k for k in ORIGIN_FIELDS if not np.array_equal(got["layers"][k], lay[k])] == []
        assert [k for k in ORIGIN_FIELDS if not np.array_equal(got["grains"][k], gr[k])] == []

        # stepping on: the map records the true transitions of the shifted lattice, and the origin map goes on from its clock
        ref.snap, ref.T_snap = np.array(f1["state"]), np.array(f1["T"])
        _step(e, calls[2:3])
        f2 = e.download()
        want_up = ref.update(f2["state"], f2["T"], 4, 1.0 / constants.VOXEL_SIZE, DT)
        up = e.solid_update(4, DT)
        assert up == want_up, (up, want_up)
        assert SOL.same_map(e.solid_read(), ref.map()) == []
        assert e.origin_seq() == seq0 + 40
    finally:
        e.close()


def test_shift_without_maps_and_with_one():
    """a handle with one map alone: the other is not touched (there is none), and ending a map behind a shift works"""
    L = 9
    e = _engine(L, 5)
    try:
        e.origin_begin()
        _step(e, batch_calls((40,)))
        w0, c0 = e.origin_words(), e.origin_census()
        e.shift((0, 0, 3))
        assert np.array_equal(e.origin_words(), SR.shift_origin_words(w0, (0, 0, 3)))
        assert np.array_equal(e.origin_census(), c0)             # d[0] = 0: the census rows stay
        assert e.origin_seq() == 40
        with pytest.raises(RuntimeError, match="needs a map"):
            e.solid_read()
        e.origin_end()
        e.solid_begin()
        e.shift((1, 1, 1))
        m = e.solid_read()
        assert (m["stamp"] == -1).all() and not _bits(m["g"]).any()
        assert e.solid_update(1, DT) == dict(n_new=0, n_cleared=0, n_recorded=0)
    finally:
        e.close()
