"""Every refusal of the thermal boundary's entry points, each made before anything is allocated or
launched and naming its entry point; and a refused call leaves the handle stepping bit-identically."""
import numpy as np
import pytest

import boundary_cases as bc
import boundary_ref as br
import remelt_cases as rc

pytestmark = pytest.mark.gpu

L = 24
CASE = rc.STEPPING["L24_laser_nolatent_rng1_incr"]
ZERO = dict(updates=0, steps=0, launches=0, coeff_uploads=0)
SINK = bc.sink(bc.COOLING)


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
    return out + [d[f].tobytes() for f in sorted(d)] + [e.implicit_info(), e.boundary_info()]


def _fresh(scheme="implicit", boundary=None):
    import cetkmc
    e = cetkmc.Engine(L, impurity_c=0.1)
    e.upload(*rc.lattice_of(CASE))
    if scheme:
        e.set_thermal_scheme(scheme)
    if boundary is not None:
        e.set_thermal_boundary(boundary)
    return e


def _with(base, field, face, value):
    b = br.boundary(base["beta"], base["T_ext"], base["ramp"])
    b[field][face] = value
    return b


def test_values_schemes_and_handles():
    import cetkmc
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    e, ex = _fresh(), _fresh(scheme=None)
    try:
        for h, fn in ((e, "cetkmc_set_thermal_boundary"), (ens, "cetkmc_ensemble_set_thermal_boundary")):
            if h is ens:
                ens.set_thermal_scheme("implicit")
            for face in (0, 3, 5):
                _refused(lambda: h.set_thermal_boundary(_with(SINK, "beta", face, -1e-300)), fn, "beta", "negative", f"face {face}")
                for bad in (np.nan, np.inf):
                    _refused(lambda: h.set_thermal_boundary(_with(SINK, "beta", face, bad)), fn, "beta", "not finite")
                for bad in (np.nan, np.inf, -np.inf):
                    _refused(lambda: h.set_thermal_boundary(_with(SINK, "T_ext", face, bad)), fn, "T_ext", "not finite")
                    _refused(lambda: h.set_thermal_boundary(_with(SINK, "ramp", face, bad)), fn, "ramp", "not finite")
            assert h.thermal_boundary() == dict(beta=[0.0] * 6, T_ext=[0.0] * 6, ramp=[0.0] * 6) and h.boundary_info() == ZERO
        # a non-adiabatic boundary needs the implicit scheme; every beta 0 does not
        _refused(lambda: ex.set_thermal_boundary(SINK), "cetkmc_set_thermal_boundary", "implicit scheme")
        ex.set_thermal_boundary(bc.BOUNDARIES["zero"])
        ex.set_thermal_boundary(None)
        ens.set_thermal_scheme("explicit")
        _refused(lambda: ens.set_thermal_boundary(SINK), "cetkmc_ensemble_set_thermal_boundary", "implicit scheme")
        ens.set_thermal_scheme("implicit")
        # the explicit scheme is refused while a non-adiabatic boundary is set
        e.set_thermal_boundary(SINK)
        ens.set_thermal_boundary(SINK)
        _refused(lambda: e.set_thermal_scheme("explicit"), "cetkmc_set_thermal_scheme", "thermal boundary")
        _refused(lambda: ens.set_thermal_scheme("explicit"), "cetkmc_ensemble_set_thermal_scheme", "thermal boundary")
        # the per-handle setter on an ensemble's handle and on its replicas; the ensemble's setter on a single handle
        for r in (0, 1):
            _refused(lambda: ens.replica(r).set_thermal_boundary(None), "cetkmc_set_thermal_boundary", "cetkmc_ensemble_set_thermal_boundary")
        lib = e.lib
        assert lib.cetkmc_set_thermal_boundary(ens.h, None) != 0 and b"cetkmc_ensemble_set_thermal_boundary" in lib.cetkmc_last_error()
        assert lib.cetkmc_ensemble_set_thermal_boundary(e.h, None) != 0 and b"not an ensemble handle" in lib.cetkmc_last_error()
        # the wrapper's own refusal of a malformed argument, by name
        with pytest.raises(ValueError, match="Engine.set_thermal_boundary"):
            e.set_thermal_boundary({"beta": [1.0] * 5})
        with pytest.raises(ValueError, match="Ensemble.set_thermal_boundary"):
            ens.set_thermal_boundary("sink")
        # back to adiabatic, then to explicit: no refusal
        e.set_thermal_boundary(None)
        e.set_thermal_scheme("explicit")
        ens.set_thermal_boundary(None)
        ens.set_thermal_scheme("explicit")
        assert e.boundary_info() == ZERO == ens.boundary_info() == e.implicit_info()
    finally:
        for h in (e, ex):
            h.close()
        ens.close()


def test_a_stepping_call_with_a_non_finite_face_temperature_is_refused_and_the_handle_steps_on():
    """ramp = -1e306 per update: T_f of update 180 (global step 3600) overflows; the calls whose own updates stay finite run.
    An adiabatic face's ramp is never evaluated."""
    import cetkmc
    hot = br.boundary(i_lo=(1.0, 2800.0, -1e306), j_hi=(0.0, 0.0, -1e308))
    assert np.isfinite(br.face_T(hot, 179)[0]) and not np.isfinite(br.face_T(hot, 180)[0])
    e, ref = _fresh(boundary=SINK), _fresh(boundary=SINK)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    try:
        e.set_thermal_boundary(hot)
        (s0, n, up, ud, unp, q) = rc.calls_of(CASE)[0]
        kw = dict(rng_mode=1, seed=3, thermal_mode=2, q_planes=q, use_latent=True)
        _refused(lambda: e.run_steps(3600, n, 0.05, up, ud, unp, **kw), "cetkmc_run_steps", "not finite", "step 3600", "face 0")
        _refused(lambda: e.run_steps(3595, n, 0.05, up, ud, unp, **kw), "cetkmc_run_steps", "not finite", "step 3600")
        assert e.boundary_info() == ZERO == e.implicit_info()         # nothing was allocated or launched
        ens.set_thermal_scheme("implicit")
        ens.set_thermal_boundary(hot)
        for r in range(2):
            ens.replica(r).upload(*rc.lattice_of(CASE))
        _refused(lambda: ens.run(3600, 3, 0.0, rng_mode=2, seeds=[1, 2], thermal_mode=1), "cetkmc_run_ensemble", "not finite", "step 3600")
        assert ens.boundary_info() == ZERO
        assert ens.run(3601, 3, 0.0, rng_mode=2, seeds=[1, 2], thermal_mode=1)["done"].tolist() == [3, 3]      # no update of its own
        e.set_thermal_boundary(SINK)
        a = _steps(e)
        assert a == _steps(ref) and a[-1]["updates"] > 0 and a[-1] == a[-2] | dict(coeff_uploads=1)
    finally:
        e.close()
        ref.close()
        ens.close()
