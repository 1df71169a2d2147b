"""cetkmc_ensemble_shift at L = 16 with R = 3 and R = 70: one record per replica, all different, one of them d = 0.

One replica is frozen (a full lattice: its first step terminates) and one is empty.  Maps are attached through the ensemble
calls and hold the records of 40 steps.  After the shift every replica's fields and info equal those of a single handle that
was given the replica's fields and the same record, its maps equal the comparator (shift_ref.py), the replica with d = 0 is
bit-identical -- fields and maps, then and after 20 more steps -- to the same replica of a twin ensemble that was never
shifted, and the frozen replica steps again."""
import numpy as np
import pytest

import shift_ref as SR
from helpers import random_lattice

pytestmark = pytest.mark.gpu

L = 16
IMPURITY_C = 0.1
DT = 1e-6
FROZEN, EMPTY, STILL = 0, 1, 2          # replica indices: frozen, empty lattice, d = 0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _lattice(r):
    st, th, ph, T, df = random_lattice(L, 50 + r)
    if r == FROZEN:
        st = np.ones_like(st)
        df = np.zeros_like(df)
    if r == EMPTY:
        st, df = np.zeros_like(st), np.zeros_like(df)
        th, ph = np.zeros_like(th), np.zeros_like(ph)
    return st, th, ph, T, df


def _record(r):
    if r == STILL:
        return None
    ds = [(-3, 0, 0), (0, 2, -5), (1, -1, 8), (0, 0, 9), (-16, 0, 0), (4, 0, 0), (0, -7, 0), (2, 3, -4)]
    return dict(d=ds[r % len(ds)], fill_state=r % 2 if r != FROZEN else 0, fill_T=2900.0 + r, T_mode=("value", "edge")[r % 3 == 1],
                fill_theta=0.01 * r, fill_phi=0.02 * r)


def _ensemble(R):
    import cetkmc
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(IMPURITY_C) for _ in range(R)])
    for r in range(R):
        ens.replica(r).upload(*_lattice(r))
    ens.solid_begin()
    ens.origin_begin()
    res = ens.run(0, 40, np.full(R, 0.02), rng_mode=2, seeds=np.arange(R) + 7, thermal_mode=1)
    ens.solid_update(1, DT)
    return ens, res


def _snapshot(ens, r):
    e = ens.replica(r)
    return dict(fields=e.download(defects=True), solid=e.solid_read(), words=e.origin_words(), seq=e.origin_seq())


def _same_fields(a, b, tag):
    for k in ("state", "defects"):
        assert np.array_equal(a[k], b[k]), (tag, k)
    for k in ("theta", "phi", "T"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)


def _same_solid(a, b, tag):
    assert np.array_equal(a["stamp"], b["stamp"]), tag
    for k in ("T_s", "g", "cool"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (tag, k)


@pytest.mark.parametrize("R", [3, 70])
def test_ensemble_shift(R):
    import cetkmc
    ens, res = _ensemble(R)
    twin, _ = _ensemble(R)
    try:
        assert res["status"][FROZEN] == 1 and res["done"][FROZEN] == 0 and (res["done"][1:] == 40).all()
        before = [_snapshot(ens, r) for r in range(R)]
        census0 = ens.origin_census()
        assert sum(int((b["solid"]["stamp"] >= 0).sum()) for b in before) > R and sum(int((b["words"] != 0).sum()) for b in before) > R
        records = [_record(r) for r in range(R)]
        infos = ens.shift(records)
        census1 = ens.origin_census()
        for r in range(R):
            tag = f"R={R} replica {r}"
            after = _snapshot(ens, r)
            if records[r] is None:
                assert infos[r] == dict(calls=0, kept=L ** 3, exposed=0, dropped=[0] * 6), tag
                _same_fields(after["fields"], before[r]["fields"], tag)
                _same_solid(after["solid"], before[r]["solid"], tag)
                assert np.array_equal(after["words"], before[r]["words"]) and np.array_equal(census1[r], census0[r]), tag
                continue
            rec = records[r]
            d = rec["d"]
            # a single handle given the replica's fields and the same record
            one = cetkmc.Engine(L, impurity_c=IMPURITY_C)
            try:
                f = before[r]["fields"]
                one.upload(f["state"], f["theta"], f["phi"], f["T"], f["defects"])
                info1 = one.shift(**rec)
                _same_fields(after["fields"], one.download(defects=True), tag)
                assert infos[r] == info1 and info1["calls"] == 1, (tag, infos[r], info1)
            finally:
                one.close()
            want, winfo = SR.shift_fields(before[r]["fields"], d, **{k: v for k, v in rec.items() if k != "d"})
            _same_fields(after["fields"], want, tag)
            assert infos[r] == dict(winfo, calls=1), tag
            _same_solid(after["solid"], SR.shift_solid(before[r]["solid"], d), tag)
            assert np.array_equal(after["words"], SR.shift_origin_words(before[r]["words"], d)), tag
            assert np.array_equal(census1[r], SR.shift_census(census0[r], d)), tag
            assert after["seq"] == before[r]["seq"], tag
        up = ens.solid_update(2, DT)
        assert not up["n_new"].any() and not up["n_cleared"].any()

        # 20 more steps: the frozen replica steps again, the replica with d = 0 is the twin's
        kw = dict(rng_mode=2, seeds=np.arange(R) + 7, thermal_mode=1)
        r2 = ens.run(40, 20, np.full(R, 0.02), **kw)
        t2 = twin.run(40, 20, np.full(R, 0.02), **kw)
        assert r2["status"][FROZEN] == 0 and r2["done"][FROZEN] == 20
        assert t2["status"][FROZEN] == 1 and t2["done"][FROZEN] == 0
        a, b = _snapshot(ens, STILL), _snapshot(twin, STILL)
        _same_fields(a["fields"], b["fields"], "d = 0 against the twin")
        assert np.array_equal(a["words"], b["words"]) and a["seq"] == b["seq"] == 60
        assert np.array_equal(_bits(r2["totals"][STILL]), _bits(t2["totals"][STILL]))
    finally:
        ens.close()
        twin.close()


def test_ensemble_refusals():
    import cetkmc
    from cetkmc import _lib
    import ctypes as C
    ens = cetkmc.Ensemble(8, [cetkmc.default_params(), cetkmc.default_params()])
    one = cetkmc.Engine(8)
    try:
        z = np.zeros((8,) * 3)
        for r in range(2):
            ens.replica(r).upload(np.zeros((8,) * 3, np.int64), z, z, z + 3000.0, None)
        before = ens.replica(0).download(defects=True)
        with pytest.raises(RuntimeError, match=r"cetkmc_ensemble_shift: .*fill_state"):
            ens.shift([dict(d=(1, 0, 0)), dict(d=(1, 0, 0), fill_state=5)])       # nothing moved in replica 0 either
        with pytest.raises(RuntimeError, match=r"cetkmc_ensemble_shift: .*T_mode"):
            ens.shift([dict(d=(1, 0, 0), T_mode=2), None])
        with pytest.raises(ValueError, match="Ensemble.shift"):
            ens.shift([None])
        assert ens.lib.cetkmc_ensemble_shift(ens.h, None, None) != 0 and b"cetkmc_ensemble_shift: null" in ens.lib.cetkmc_last_error()
        buf = (_lib.Shift * 2)()
        assert ens.lib.cetkmc_ensemble_shift(one.h, buf, None) != 0
        assert b"cetkmc_ensemble_shift: not an ensemble handle" in ens.lib.cetkmc_last_error()
        buf[1].pad = 1
        assert ens.lib.cetkmc_ensemble_shift(ens.h, buf, None) != 0 and b"pad" in ens.lib.cetkmc_last_error()
        _same_fields(ens.replica(0).download(defects=True), before, "after the refusals")
        assert [i["calls"] for i in ens.shift([None, dict(d=(0, 0, 1))])] == [0, 1]
        # a replica handle goes to the single call
        assert ens.replica(1).shift((0, 1, 0))["calls"] == 2
        assert C.sizeof(_lib.Shift) == 48
    finally:
        ens.close()
        one.close()
