"""Every refusal of the implicit scheme's entry points and of the calls the scheme bars, each made before anything is allocated
or launched and naming its entry point; and a refused call leaves the handle stepping bit-identically."""
import pytest

import remelt_cases as rc

pytestmark = pytest.mark.gpu

L = 24
CASE = rc.STEPPING["L24_laser_nolatent_rng1_incr"]
ZERO = dict(updates=0, steps=0, launches=0, coeff_uploads=0)


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
    return out + [d[f].tobytes() for f in sorted(d)] + [e.implicit_info()]


def _fresh(scheme=None, **kw):
    import cetkmc
    e = cetkmc.Engine(L, impurity_c=0.1, **kw)
    e.upload(*rc.lattice_of(CASE))
    if scheme:
        e.set_thermal_scheme(scheme)
    return e


def test_values_and_handles():
    import cetkmc
    rank = cetkmc.Engine(L, impurity_c=0.1, rank=0, nranks=1, host_comm=(lambda *a: 0, lambda *a: 0))
    slabs = _fresh(n_slabs=3)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    e = _fresh()
    try:
        for bad in (2, -1, 2 ** 31 - 1):
            _refused(lambda: e.set_thermal_scheme(bad), "cetkmc_set_thermal_scheme", "unknown thermal scheme")
            _refused(lambda: ens.set_thermal_scheme(bad), "cetkmc_ensemble_set_thermal_scheme", "unknown thermal scheme")
        for bad in ("crank-nicolson", "Implicit", None, 1.0, True, ["implicit"]):      # the wrapper's own refusal, by name
            with pytest.raises(ValueError, match="Engine.set_thermal_scheme"):
                e.set_thermal_scheme(bad)
            with pytest.raises(ValueError, match="Ensemble.set_thermal_scheme"):
                ens.set_thermal_scheme(bad)
        _refused(lambda: rank.set_thermal_scheme("implicit"), "cetkmc_set_thermal_scheme", "one slab of one process")
        _refused(lambda: slabs.set_thermal_scheme("implicit"), "cetkmc_set_thermal_scheme", "one slab of one process")
        for r in (0, 1):
            _refused(lambda: ens.replica(r).set_thermal_scheme("implicit"), "cetkmc_set_thermal_scheme", "cetkmc_ensemble_set_thermal_scheme")
        lib = e.lib
        assert lib.cetkmc_set_thermal_scheme(ens.h, 1) != 0 and b"cetkmc_ensemble_set_thermal_scheme" in lib.cetkmc_last_error()
        assert lib.cetkmc_ensemble_set_thermal_scheme(e.h, 1) != 0 and b"cetkmc_ensemble_set_thermal_scheme" in lib.cetkmc_last_error()
        # no refusals: the explicit scheme on any single handle, either scheme on an ensemble, and back
        rank.set_thermal_scheme("explicit")
        slabs.set_thermal_scheme(0)
        e.set_thermal_scheme("implicit")
        e.set_thermal_scheme("explicit")
        ens.set_thermal_scheme("implicit")
        ens.set_thermal_scheme("explicit")
        assert e.implicit_info() == ZERO == ens.implicit_info() == slabs.implicit_info()
    finally:
        for h in (e, rank, slabs):
            h.close()
        ens.close()


def test_lookahead_and_the_implicit_scheme_exclude_each_other():
    e, ref = _fresh(), _fresh("implicit")
    try:
        e.set_option("thermal_lookahead", 1)
        _refused(lambda: e.set_thermal_scheme("implicit"), "cetkmc_set_thermal_scheme", "thermal_lookahead")
        e.set_thermal_scheme("explicit")                  # what the handle has
        e.set_option("thermal_lookahead", 0)
        e.set_thermal_scheme("implicit")
        _refused(lambda: e.set_option("thermal_lookahead", 1), "cetkmc_set_option", "thermal_lookahead", "implicit")
        e.set_option("thermal_lookahead", 0)
        assert e.implicit_info() == ZERO                  # nothing was allocated or launched
        a = _steps(e)
        assert a == _steps(ref) and a[-1]["updates"] > 0
    finally:
        e.close()
        ref.close()


def test_mode_b_is_barred_while_the_scheme_is_implicit_and_the_handle_steps_on():
    e, ref = _fresh("implicit"), _fresh("implicit")
    try:
        _refused(lambda: e.run_supersteps(0, 3, 8, 0.0, 1), "cetkmc_run_supersteps", "implicit")
        _refused(lambda: e.run_supersteps(0, 3, L, 0.0, 1), "cetkmc_run_supersteps", "implicit")      # box == L as well
        _refused(lambda: e.run_supersteps_local(0, 3, 0.0, 1, 4, 2.0), "cetkmc_run_supersteps_local", "implicit")
        _refused(lambda: e.set_thermal_scheme(7), "cetkmc_set_thermal_scheme")
        assert e.implicit_info() == ZERO                  # nothing was launched
        a, b = _steps(e), _steps(ref)
        assert a == b and a[-1]["updates"] > 0 and a[-1]["launches"] == 3 * a[-1]["updates"]
        # with the scheme back at explicit the super-steps run again
        e.set_thermal_scheme("explicit")
        assert e.run_supersteps(40, 2, 8, 0.0, 1)["done"] == 2
    finally:
        e.close()
        ref.close()
