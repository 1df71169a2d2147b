"""Everything cetkmc_run_supersteps_local refuses, each with a cetkmc_last_error text, and that a refused call leaves the
lattice alone."""
import math

import numpy as np
import pytest

from helpers import random_lattice

pytestmark = pytest.mark.gpu


def _refused(e, match, **kw):
    args = dict(step0=0, n=2, defect_fraction=0.0, seed=1, max_events=4, horizon_events=1.0)
    args.update(kw)
    with pytest.raises(RuntimeError, match=match):
        e.run_supersteps_local(**args)


def _raw(e, box):
    import ctypes as C

    from cetkmc import _lib
    a, res = _lib.LocalArgs(), _lib.RunResult()
    a.step0, a.n_steps, a.box, a.seed, a.thermal_mode, a.thermal_dt, a.max_events, a.horizon_events = 0, 1, box, 1, 1, 1e-6, 4, 1.0
    rc = e.lib.cetkmc_run_supersteps_local(e.h, C.byref(a), C.byref(res), None, None, None, None, None, None)
    return rc, e.error()


def test_argument_refusals():
    import cetkmc
    L = 16
    fields = random_lattice(L, 3, fill=0.2)
    e = cetkmc.Engine(L, impurity_c=0.2)
    e.upload(*fields)
    before = e.download()
    for box in (4, 10, 16):
        rc, msg = _raw(e, box)
        assert rc != 0 and "box must be 8" in msg
    for K in (0, -1, 65):
        _refused(e, "max_events", max_events=K)
    for hor in (0.0, -1.0, math.nan, -math.inf):
        _refused(e, "horizon_events", horizon_events=hor)
    _refused(e, "thermal_mode 2", thermal_mode=2)
    e.set_option("sweep_variant", 0)
    _refused(e, "sweep_variant")
    e.set_option("sweep_variant", 1)
    after = e.download()
    for f in before:
        assert np.array_equal(before[f], after[f], equal_nan=True), f
    r = e.run_supersteps_local(0, 2, 0.0, 1, 4, math.inf)           # an infinite horizon is accepted
    assert r["done"] == 2 and np.all(np.isinf(r["horizon"]))
    e.close()
    e = cetkmc.Engine(20, impurity_c=0.2)                            # L % 8 != 0
    e.upload(*random_lattice(20, 3, fill=0.2))
    rc, msg = _raw(e, 8)
    assert rc != 0 and "box must be 8 and divide L" in msg
    e.close()


def test_handle_refusals():
    import cetkmc
    L = 16
    fields = random_lattice(L, 3, fill=0.2)
    e = cetkmc.Engine(L, impurity_c=0.2, n_slabs=2)
    e.upload(*fields)
    _refused(e, "one slab")
    e.close()
    e = cetkmc.Engine(L, impurity_c=0.2, rank=0, nranks=1, unique_id=cetkmc.Engine.unique_id())
    e.upload(*fields)
    _refused(e, "one slab of one process")
    e.close()
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.2)] * 2)
    rep = ens.replica(0)
    rep.upload(*fields)
    _refused(rep, "ensemble replica")
    ens.close()
