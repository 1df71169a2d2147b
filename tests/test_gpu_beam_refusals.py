"""Every refusal of the beam tables' entry points, each made before anything is allocated or launched and
naming its entry point; and a refused call leaves the handle stepping bit-identically."""
import numpy as np
import pytest

import beam_cases as bm
import implicit_cases as ic
import remelt_cases as rc

pytestmark = pytest.mark.gpu

L = 24
CASE = bm.STEPPING["L24_nolatent_rng1_incr_n1_D4"]
ZERO = dict(updates=0, steps=0, launches=0, table_uploads=0)


def _table(u0=0, n_u=4, D=2, **over):
    t = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in bm.scan_table(L, u0, n_u, D).items()}
    for k, (idx, v) in over.items():
        t[k].flat[idx] = v
    return t


def _refused(call, *words):
    with pytest.raises(RuntimeError) as err:
        call()
    for w in words:
        assert w in str(err.value), (w, str(err.value))


def _steps(e):
    """two calls of the case with the handle's table; everything they return and leave, as bytes"""
    out = []
    for (s0, n, up, ud, unp, _) in bm.calls_of(CASE)[:2]:
        r = e.run_steps(s0, n, 0.05, up, ud, unp, rng_mode=1, seed=3, thermal_mode=2, use_latent=True)
        out += [r["done"], r["status"], r["np_used"], r["q_used"], r["totals"].tobytes(), r["events"].tobytes()]
    d = e.download(defects=True)
    return out + [d[f].tobytes() for f in sorted(d)] + [e.implicit_info(), e.beam_info()]


def _fresh(scheme="implicit", table=None):
    import cetkmc
    e = cetkmc.Engine(L, impurity_c=0.1)
    e.upload(*ic.lattice_of(CASE))
    if scheme:
        e.set_thermal_scheme(scheme)
    if table is not None:
        e.set_beam(table)
    return e


def _raw(e, **fields):
    """cetkmc_set_beam with a hand-made struct (what the wrapper's shape checks would stop)"""
    from cetkmc import engine
    keep = []
    b = engine._beam_struct(_table(), L, "x", keep)
    for k, v in fields.items():
        setattr(b, k, v)
    rc_ = e.lib.cetkmc_set_beam(e.h, b)
    return rc_, e.lib.cetkmc_last_error().decode()


def test_tables_schemes_and_handles():
    import cetkmc
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    e, ex = _fresh(), _fresh(scheme=None)
    try:
        ens.set_thermal_scheme("implicit")
        # a bad table: n_u < 1, depth outside 1..L, a null array, a negative or non-finite value
        for fields, word in ((dict(n_u=0), "n_u"), (dict(depth=0), "depth"), (dict(depth=L + 1), "depth"), (dict(amp=None), "required"),
                             (dict(gj=None), "required"), (dict(gk=None), "required"), (dict(fi=None), "required")):
            rc_, err = _raw(e, **fields)
            assert rc_ != 0 and "cetkmc_set_beam" in err and word in err, (fields, err)
        for f in ("amp", "gj", "gk", "fi"):
            for bad in (-1e-300, np.nan, np.inf, -np.inf):
                _refused(lambda: e.set_beam(_table(**{f: (1, bad)})), "cetkmc_set_beam", f + "[1]", "negative or not finite")
                _refused(lambda: ens.set_beam([_table(), _table(**{f: (1, bad)})]), "cetkmc_ensemble_set_beam", "set 1", f + "[1]")
        assert e.beam_info() == ZERO == ens.beam_info()
        # a beam needs the implicit scheme
        _refused(lambda: ex.set_beam(_table()), "cetkmc_set_beam", "implicit scheme")
        ex.set_beam(None)
        ens.set_thermal_scheme("explicit")
        _refused(lambda: ens.set_beam([_table(), _table()]), "cetkmc_ensemble_set_beam", "implicit scheme")
        ens.set_thermal_scheme("implicit")
        # ensemble tables: sets that disagree in u0, n_u or depth; set_of outside [0, n_sets); no set_of and n_sets != R
        for other in (_table(u0=1), _table(n_u=3), _table(D=3)):
            _refused(lambda: ens.set_beam([_table(), other]), "cetkmc_ensemble_set_beam", "set 1", "u0, n_u or depth")
        for so in ([0, 2], [-1, 0]):
            _refused(lambda: ens.set_beam([_table(), _table()], so), "cetkmc_ensemble_set_beam", "set_of", "outside")
        _refused(lambda: ens.set_beam([_table()]), "cetkmc_ensemble_set_beam", "n_sets must equal R")
        with pytest.raises(ValueError, match="Ensemble.set_beam"):
            ens.set_beam([_table()], [0])
        assert ens.beam_info() == ZERO
        # the explicit scheme is refused while a beam is set
        e.set_beam(_table())
        ens.set_beam([_table()], [0, 0])
        _refused(lambda: e.set_thermal_scheme("explicit"), "cetkmc_set_thermal_scheme", "beam")
        _refused(lambda: ens.set_thermal_scheme("explicit"), "cetkmc_ensemble_set_thermal_scheme", "beam")
        # the per-handle setter on an ensemble's handle and on its replicas; the ensemble's setter on a single handle
        for r in (0, 1):
            _refused(lambda: ens.replica(r).set_beam(None), "cetkmc_set_beam", "cetkmc_ensemble_set_beam")
        lib = e.lib
        assert lib.cetkmc_set_beam(ens.h, None) != 0 and b"cetkmc_ensemble_set_beam" in lib.cetkmc_last_error()
        assert lib.cetkmc_ensemble_set_beam(e.h, 0, None, None) != 0 and b"not an ensemble handle" in lib.cetkmc_last_error()
        with pytest.raises(ValueError, match="Engine.set_beam"):
            e.set_beam({"amp": [1.0]})
        # removed, then explicit: no refusal
        e.set_beam(None)
        e.set_thermal_scheme("explicit")
        ens.set_beam(None)
        ens.set_thermal_scheme("explicit")
        assert e.beam_info() == dict(ZERO, table_uploads=1) == ens.beam_info()
    finally:
        for h in (e, ex):
            h.close()
        ens.close()


def test_refused_calls_leave_the_handle_stepping_on():
    """planes beside a beam, updates outside the table (from step0 and n_steps, before the first launch), cetkmc_thermal_laser and
    a direct update outside the table, cetkmc_thermal_beam without a table: refused; then the handle steps like a fresh one"""
    import cetkmc
    t = _table(u0=0, n_u=4, D=4)
    e, ref, bare = _fresh(table=t), _fresh(table=t), _fresh()
    ens = cetkmc.Ensemble(L, [cetkmc.default_params(0.1)] * 2)
    try:
        (s0, n, up, ud, unp, _) = bm.calls_of(CASE)[0]
        kw = dict(rng_mode=1, seed=3, thermal_mode=2, use_latent=True)
        q = np.zeros((1, L, L))
        _refused(lambda: e.run_steps(0, n, 0.05, up, ud, unp, q_planes=q, **kw), "cetkmc_run_steps", "q_planes must be NULL")
        _refused(lambda: e.stage_inputs(0, n, 0.05, up, ud, unp, q_planes=q, **kw), "cetkmc_stage_inputs", "q_planes must be NULL")
        # updates 0..3 are in the table: step 80 is ordinal 4
        _refused(lambda: e.run_steps(75, n, 0.05, up, ud, unp, **kw), "cetkmc_run_steps", "ordinals 4 to 4", "[0, 4)")
        _refused(lambda: e.run_steps(61, 20, 0.05, up, ud, unp, **kw), "cetkmc_run_steps", "ordinals 4 to 4")
        _refused(lambda: e.thermal_beam(1e-6, 4), "cetkmc_thermal_beam", "ordinal 4", "[0, 4)")
        _refused(lambda: e.thermal_beam(1e-6, -1), "cetkmc_thermal_beam", "ordinal -1")
        _refused(lambda: e.thermal_laser(1e-6, q[0]), "cetkmc_thermal_laser", "beam is set")
        _refused(lambda: bare.thermal_beam(1e-6, 0), "cetkmc_thermal_beam", "no beam is set")
        assert e.beam_info() == dict(ZERO, table_uploads=1) and e.implicit_info()["updates"] == 0        # nothing was launched
        ens.set_thermal_scheme("implicit")
        ens.set_beam([t], [0, 0])
        for r in range(2):
            ens.replica(r).upload(*rc.lattice_of(CASE))
        ekw = dict(rng_mode=2, seeds=[1, 2], thermal_mode=2)
        _refused(lambda: ens.run(80, 3, 0.0, **ekw), "cetkmc_run_ensemble", "ordinals 4 to 4")
        _refused(lambda: ens.run(0, 3, 0.0, q_planes=np.zeros((2, 1, L, L)), **ekw), "cetkmc_run_ensemble", "q_planes must be NULL")
        assert ens.beam_info() == dict(ZERO, table_uploads=1)
        assert ens.run(81, 3, 0.0, **ekw)["done"].tolist() == [3, 3]          # no update of its own
        a = _steps(e)
        assert a == _steps(ref) and a[-1]["updates"] > 0
    finally:
        for h in (e, ref, bare):
            h.close()
        ens.close()
