"""Every refusal of the remelting entry points and of the calls remelting bars, each made before anything is launched and
naming its entry point; and a refused call leaves the handle stepping bit-identically."""
import ctypes as C

import numpy as np
import pytest

import remelt_cases as rc

pytestmark = pytest.mark.gpu

L = 24
CASE = rc.STEPPING["L24_laser_nolatent_rng1_incr"]
THR = rc.T_MELT


def _refused(call, *words):
    with pytest.raises(RuntimeError) as err:
        call()
    for w in words:
        assert w in str(err.value), (w, str(err.value))


def _steps(e):
    """two calls of the case with whatever the handle's remelt setting is; everything they return and leave, as bytes"""
    out = []
    for (s0, n, up, ud, unp, q) in rc.calls_of(CASE)[:2]:
        r = e.run_steps(s0, n, 0.05, up, ud, unp, rng_mode=1, seed=3, thermal_mode=2, q_planes=q, use_latent=True)
        out += [r["done"], r["status"], r["np_used"], r["totals"].tobytes(), r["events"].tobytes()]
    d = e.download(defects=True)
    return out + [d[f].tobytes() for f in sorted(d)] + [e.remelt_info()]


def _fresh(remelt):
    import cetkmc
    e = cetkmc.Engine(L, impurity_c=0.1)
    e.upload(*rc.lattice_of(CASE))
    if remelt:
        e.set_remelt(True, THR)
    return e


def test_handles_and_thresholds():
    import cetkmc
    two = cetkmc.Engine(L, impurity_c=0.1, n_slabs=2)
    rank = cetkmc.Engine(L, impurity_c=0.1, rank=0, nranks=1, host_comm=(lambda *a: 0, lambda *a: 0))
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    e = _fresh(False)
    try:
        for h in (two, rank):
            _refused(lambda: h.set_remelt(True, THR), "cetkmc_set_remelt", "one slab")
            _refused(lambda: h.remelt(THR), "cetkmc_remelt", "one slab")
        _refused(lambda: e.set_remelt(True, float("nan")), "cetkmc_set_remelt", "NaN")
        _refused(lambda: e.remelt(float("nan")), "cetkmc_remelt", "NaN")
        _refused(lambda: ens.set_remelt(True, float("nan")), "cetkmc_ensemble_set_remelt", "NaN")
        _refused(lambda: ens.replica(0).set_remelt(True, THR), "cetkmc_set_remelt", "cetkmc_ensemble_set_remelt")
        _refused(lambda: ens.replica(1).set_remelt(True, THR), "cetkmc_set_remelt", "cetkmc_ensemble_set_remelt")
        lib = e.lib
        assert lib.cetkmc_ensemble_set_remelt(e.h, 1, C.c_double(THR)) != 0 and b"cetkmc_ensemble_set_remelt" in lib.cetkmc_last_error()
        info = cetkmc._lib.RemeltInfo()
        assert lib.cetkmc_ensemble_remelt_info(e.h, C.byref(info)) != 0 and b"cetkmc_ensemble_remelt_info" in lib.cetkmc_last_error()
        # thresholds that are no refusals: the infinities, and switching off with anything finite
        e.set_remelt(True, float("inf"))
        e.set_remelt(True, float("-inf"))
        e.set_remelt(False, 0.0)
        assert e.remelt_info() == dict(passes=0, n_melted=0, n_melted_last=0, n_appended=0)
    finally:
        for h in (e, two, rank):
            h.close()
        ens.close()


def test_calls_barred_while_remelting_is_on_and_the_handle_steps_on():
    e, ref = _fresh(True), _fresh(True)
    try:
        _refused(lambda: e.run_supersteps(0, 3, 8, 0.0, 1), "cetkmc_run_supersteps", "remelting is on")
        _refused(lambda: e.run_supersteps(0, 3, L, 0.0, 1), "cetkmc_run_supersteps", "remelting is on")      # box == L as well
        _refused(lambda: e.run_supersteps_local(0, 3, 0.0, 1, 4, 2.0), "cetkmc_run_supersteps_local", "remelting is on")
        _refused(lambda: e.set_option("thermal_lookahead", 1), "cetkmc_set_option", "thermal_lookahead")
        _refused(e.origin_begin, "cetkmc_origin_begin", "remelting is on")
        _refused(lambda: e.set_remelt(True, float("nan")), "cetkmc_set_remelt", "NaN")
        e.set_option("thermal_lookahead", 0)
        assert e.origin_seq() == -1
        assert _steps(e) == _steps(ref)
        assert e.remelt_info()["n_melted"] > 0
    finally:
        e.close()
        ref.close()


def test_origin_map_and_lookahead_bar_remelting_and_the_handle_steps_on():
    e, ref = _fresh(False), _fresh(False)
    try:
        for h in (e, ref):
            h.origin_begin()
        _refused(lambda: e.set_remelt(True, THR), "cetkmc_set_remelt", "origin map")
        _refused(lambda: e.remelt(THR), "cetkmc_remelt", "origin map")
        e.set_remelt(False, THR)                       # switching off is no refusal
        assert _steps(e) == _steps(ref)
        assert e.origin_words().tobytes() == ref.origin_words().tobytes() and e.remelt_info()["passes"] == 0
        for h in (e, ref):
            h.origin_end()
        e.set_option("thermal_lookahead", 1)
        _refused(lambda: e.set_remelt(True, THR), "cetkmc_set_remelt", "thermal_lookahead")
        e.set_option("thermal_lookahead", 0)
        e.set_remelt(True, THR)                        # and now it is accepted
        ref.set_remelt(True, THR)
        _refused(e.origin_begin, "cetkmc_origin_begin", "remelting is on")
    finally:
        e.close()
        ref.close()


def test_ensemble_refusals():
    import cetkmc
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    try:
        for r in range(2):
            ens.replica(r).upload(*rc.lattice_of(CASE, r))
        ens.origin_begin()
        _refused(lambda: ens.set_remelt(True, THR), "cetkmc_ensemble_set_remelt", "origin map")
        _refused(lambda: ens.replica(1).remelt(THR), "cetkmc_remelt", "origin map")
        ens.origin_end()
        ens.set_remelt(True, THR)
        _refused(ens.origin_begin, "cetkmc_ensemble_origin_begin", "remelting is on")
        ens.set_remelt(False, THR)
        ens.origin_begin()
        ens.origin_end()
    finally:
        ens.close()
