"""Every refusal of cetkmc_shift (include/cetkmc.h): a NULL record, fill_state outside 0..4, an unknown T_mode, a non-zero pad,
a handle with several slabs, a rank handle.  Each names its entry point, comes before anything is allocated or launched -- the
counters do not move -- and leaves the handle usable with its fields unchanged.  Non-finite fills are accepted.  (The
ensemble call's refusals are in test_gpu_shift_ensemble.py.)"""
import ctypes as C

import numpy as np
import pytest

import shift_ref as SR
from helpers import random_lattice

pytestmark = pytest.mark.gpu

L = 12


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("state", "defects")) and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in ("theta", "phi", "T"))


def test_records():
    import cetkmc
    from cetkmc import _lib, engine
    e = cetkmc.Engine(L, impurity_c=0.1)
    try:
        e.upload(*random_lattice(L, 4))
        e.rate_sweep()
        before, c0 = e.download(defects=True), e.counters()
        bad = [(dict(fill_state=-1), "fill_state"), (dict(fill_state=5), "fill_state"), (dict(T_mode=2), "T_mode"), (dict(T_mode=-1), "T_mode")]
        for kw, what in bad:
            with pytest.raises(RuntimeError, match=r"cetkmc_shift: .*" + what):
                e.shift((1, 0, 0), **kw)
        s = engine._shift_struct((1, 0, 0))
        s.pad = 7
        assert e.lib.cetkmc_shift(e.h, C.byref(s), None) != 0 and e.error().startswith("cetkmc_shift: ") and "pad" in e.error()
        assert e.lib.cetkmc_shift(e.h, None, None) != 0 and e.error().startswith("cetkmc_shift: null")
        info = _lib.ShiftInfo()
        assert e.lib.cetkmc_shift(None, C.byref(s), C.byref(info)) != 0 and e.error().startswith("cetkmc_shift: null")
        # a record that is wrong is refused even where d = 0 would have made it a no-op
        with pytest.raises(RuntimeError, match="cetkmc_shift: .*fill_state"):
            e.shift((0, 0, 0), fill_state=9)
        c1 = e.counters()
        assert c1 == c0 and e.counters()["sweeps"] == c0["sweeps"]
        e.row_sums()                                         # the sweep cache survived the refusals
        assert _same(e.download(defects=True), before)
        # usable, and non-finite fills are the lattice's to hold
        info = e.shift((0, -2, 1), fill_state=4, fill_T=np.nan, fill_theta=np.inf, fill_phi=-np.inf, T_mode=0)
        want, winfo = SR.shift_fields(before, (0, -2, 1), fill_state=4, fill_T=np.nan, fill_theta=np.inf, fill_phi=-np.inf)
        assert info == dict(winfo, calls=1) and _same(e.download(defects=True), want)
        with pytest.raises(RuntimeError, match="needs a preceding cetkmc_rate_sweep"):
            e.row_sums()                                     # as behind an upload: the sweep cache is stale
        assert e.lib.cetkmc_shift(e.h, C.byref(engine._shift_struct((1, 0, 0))), None) == 0      # info may be NULL
        assert e.shift((0, 0, 0))["calls"] == 2              # ... and the call counted
    finally:
        e.close()


def test_handles():
    import cetkmc
    fields = random_lattice(L, 5)
    slabs = cetkmc.Engine(L, impurity_c=0.1, n_slabs=2)
    rank = cetkmc.Engine(L, impurity_c=0.1, rank=0, nranks=1, host_comm=(lambda *a: 0, lambda *a: 0))
    try:
        for e in (slabs, rank):
            e.upload(*fields)
            before, c0 = e.download(defects=True), e.counters()
            with pytest.raises(RuntimeError, match="cetkmc_shift needs the whole lattice in one slab of one process"):
                e.shift((1, 0, 0))
            with pytest.raises(RuntimeError, match="cetkmc_shift"):
                e.shift((0, 0, 0))                           # also where nothing would move
            assert e.counters() == c0 and _same(e.download(defects=True), before)
            assert e.rate_sweep()[1] > 0
    finally:
        slabs.close()
        rank.close()
