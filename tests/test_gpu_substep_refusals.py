"""Every refusal of the sub-stepping entry points and of the calls sub-stepping bars, each made before anything is launched
and naming its entry point; and a refused call leaves the handle stepping bit-identically."""
import pytest

import remelt_cases as rc

pytestmark = pytest.mark.gpu

L = 24
CASE = rc.STEPPING["L24_laser_nolatent_rng1_incr"]
ZERO = dict(updates=0, substeps=0, launches=0, blocked_launches=0)


def _refused(call, *words):
    with pytest.raises(RuntimeError) as err:
        call()
    for w in words:
        assert w in str(err.value), (w, str(err.value))


def _steps(e):
    """two calls of the case with whatever the handle's setting is; everything they return and leave, as bytes"""
    out = []
    for (s0, n, up, ud, unp, q) in rc.calls_of(CASE)[:2]:
        r = e.run_steps(s0, n, 0.05, up, ud, unp, rng_mode=1, seed=3, thermal_mode=2, q_planes=q, use_latent=True)
        out += [r["done"], r["status"], r["np_used"], r["totals"].tobytes(), r["events"].tobytes()]
    d = e.download(defects=True)
    return out + [d[f].tobytes() for f in sorted(d)] + [e.substep_info()]


def _fresh(n_sub=None):
    import cetkmc
    e = cetkmc.Engine(L, impurity_c=0.1)
    e.set_option("substep_block", 3)           # the blocked kernel (the default at this size is one launch per sub-step)
    e.upload(*rc.lattice_of(CASE))
    if n_sub:
        e.set_thermal_substeps(n_sub)
    return e


def test_counts_and_handles():
    import cetkmc
    rank = cetkmc.Engine(L, impurity_c=0.1, rank=0, nranks=1, host_comm=(lambda *a: 0, lambda *a: 0))
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    e = _fresh()
    try:
        for n in (0, -1, -2 ** 31):
            _refused(lambda: e.set_thermal_substeps(n), "cetkmc_set_thermal_substeps", ">= 1")
            _refused(lambda: ens.set_thermal_substeps(n), "cetkmc_ensemble_set_thermal_substeps", ">= 1")
        _refused(lambda: e.set_thermal_substeps(65537), "cetkmc_set_thermal_substeps", "65536")
        _refused(lambda: ens.set_thermal_substeps(2 ** 31 - 1), "cetkmc_ensemble_set_thermal_substeps", "65536")
        for n in (1, 2):
            _refused(lambda: rank.set_thermal_substeps(n), "cetkmc_set_thermal_substeps", "rank handle")
        _refused(lambda: ens.replica(0).set_thermal_substeps(2), "cetkmc_set_thermal_substeps", "cetkmc_ensemble_set_thermal_substeps")
        _refused(lambda: ens.replica(1).set_thermal_substeps(2), "cetkmc_set_thermal_substeps", "cetkmc_ensemble_set_thermal_substeps")
        lib = e.lib
        assert lib.cetkmc_set_thermal_substeps(ens.h, 2) != 0 and b"cetkmc_ensemble_set_thermal_substeps" in lib.cetkmc_last_error()
        assert lib.cetkmc_ensemble_set_thermal_substeps(e.h, 2) != 0 and b"cetkmc_ensemble_set_thermal_substeps" in lib.cetkmc_last_error()
        for key, bad in (("substep_block", -1), ("substep_block", 5), ("substep_planes", -1)):
            _refused(lambda: e.set_option(key, bad), key)
        # no refusals: the cap itself, and back to 1
        e.set_thermal_substeps(65536)
        e.set_thermal_substeps(1)
        ens.set_thermal_substeps(3)
        ens.set_thermal_substeps(1)
        assert e.substep_info() == ZERO == ens.substep_info()
    finally:
        for h in (e, rank):
            h.close()
        ens.close()


def test_lookahead_and_substeps_exclude_each_other():
    e, ref = _fresh(), _fresh()
    try:
        e.set_option("thermal_lookahead", 1)
        _refused(lambda: e.set_thermal_substeps(2), "cetkmc_set_thermal_substeps", "thermal_lookahead")
        e.set_thermal_substeps(1)                         # n = 1 is what the handle has
        e.set_option("thermal_lookahead", 0)
        e.set_thermal_substeps(2)
        _refused(lambda: e.set_option("thermal_lookahead", 1), "cetkmc_set_option", "thermal_lookahead", "thermal_substeps")
        e.set_option("thermal_lookahead", 0)
        ref.set_thermal_substeps(2)
        assert _steps(e) == _steps(ref)
    finally:
        e.close()
        ref.close()


def test_calls_barred_while_substepping_and_the_handle_steps_on():
    e, ref = _fresh(17), _fresh(17)
    try:
        _refused(lambda: e.run_supersteps(0, 3, 8, 0.0, 1), "cetkmc_run_supersteps", "thermal_substeps")
        _refused(lambda: e.run_supersteps(0, 3, L, 0.0, 1), "cetkmc_run_supersteps", "thermal_substeps")      # box == L as well
        _refused(lambda: e.run_supersteps_local(0, 3, 0.0, 1, 4, 2.0), "cetkmc_run_supersteps_local", "thermal_substeps")
        _refused(lambda: e.set_thermal_substeps(0), "cetkmc_set_thermal_substeps")
        _refused(lambda: e.set_option("thermal_lookahead", 1), "cetkmc_set_option")
        assert e.substep_info() == ZERO                   # nothing was launched
        a, b = _steps(e), _steps(ref)
        assert a == b and a[-1]["updates"] > 0 and a[-1]["blocked_launches"] > 0
        # with n back at 1 the super-steps run again
        e.set_thermal_substeps(1)
        assert e.run_supersteps(40, 2, 8, 0.0, 1)["done"] == 2
    finally:
        e.close()
        ref.close()
