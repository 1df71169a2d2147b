"""What a mutating call makes stale, seen from outside: too little and too much.

Every case starts from a handle with every cache fresh (a warm cetkmc_rate_sweep) and a staged batch, applies ONE cause
and then reads what the library already shows:

  SWEEP   cetkmc_row_sums is refused exactly when the cause makes the row sums stale
  TABLE   the next cetkmc_rate_sweep rewrites the rate table (counter table_updates + 1) exactly when it is stale
  IFC     ... and re-evaluates the interface list (interface_launches + 1) exactly when the table or the list's sums are
  STAGED  cetkmc_run_steps without input pointers is accepted exactly when the staged batch survived

The expectations are the rows of tests/test_invalidation_table_host.py, written out by hand and not read from the library:
this test passed unchanged on the library as it was before its table existed, when every site set its flags itself.
One slab and two slabs on one device: cetkmc_set_prev_state works slab by slab."""
import numpy as np
import pytest

import live_ops as lo
from test_invalidation_table_host import IFC, STAGED, SWEEP, TABLE, TABLE_

pytestmark = pytest.mark.gpu

L = 24
N_STAGED = 2
_FIELDS = {}


def _fields(seed):
    if seed not in _FIELDS:
        _FIELDS[seed] = lo.fields(L, seed)
    return _FIELDS[seed]


def _batch(n):
    rs = np.random.RandomState(31)
    return dict(step0=1, n=n, defect_fraction=lo.DEFECT_FRACTION, u_pick=rs.random_sample(n), u_defect=rs.random_sample(n),
                u_np=rs.random_sample(2 * n + 2), rng_mode=1, seed=lo.COUNTER_SEED, thermal_mode=0)


def _upload(**which):
    names = ("state", "theta", "phi", "T", "defects")
    return lambda e: e.upload(**{k: _fields(1)[names.index(k)] for k in which})


def _option(key, value):
    return lambda e: e.set_option(key, value)


def _set_params(e):
    e.params.I0 = lo.ALT_PARAMS["I0"]
    e.set_params()


def _apply(e):
    total, _, _ = e.rate_sweep()
    e.apply(e.select(0.37 * total), 0.3, 0.4, True)


def _laser(e):
    from cetkmc import synthetic
    e.thermal_laser(lo.THERMAL_DT, synthetic.laser_planes(L, 0, 1, power=lo.LASER_POWER)[0], use_latent=True, scrub_nan=True)


def _sparse(e):
    e.set_defects_sparse(np.arange(0, L ** 3, 7, dtype=np.int64))


# (case, cause of the table or None for a call that must leave every cache alone, the call).  At L = 24 the temperature
# update runs the marching kernel, which does not write the table
CASES = [
    ("upload_state", "upload_T_or_state", _upload(state=1)),
    ("upload_theta", "upload", _upload(theta=1)),
    ("upload_phi", "upload", _upload(phi=1)),
    ("upload_T", "upload_T_or_state", _upload(T=1)),
    ("upload_defects", "upload", _upload(defects=1)),
    ("upload_all", "upload_T_or_state", _upload(state=1, theta=1, phi=1, T=1, defects=1)),
    ("set_params", "set_params", _set_params),
    ("opt_sweep_variant", "option_sweep_variant", _option("sweep_variant", 1)),
    ("opt_interface_every_step", "option_interface_every_step", _option("interface_every_step", 0)),
    ("opt_reserve_batch", "option_reserve_batch", _option("reserve_batch", 64)),
    ("opt_apply_in_sweep", None, _option("apply_in_sweep", 0)),
    ("opt_fused_tiles", None, _option("fused_tiles", 2)),
    ("opt_thermal_variant", None, _option("thermal_variant", 2)),
    ("opt_thermal_planes_per_block", None, _option("thermal_planes_per_block", 3)),
    ("opt_thermal_planes_per_block16", None, _option("thermal_planes_per_block16", 5)),
    ("opt_thermal_lookahead", None, _option("thermal_lookahead", 1)),
    ("opt_thermal_table", None, _option("thermal_table", 0)),
    ("set_defects", "set_defects", lambda e: e.set_defects(lo.defect_mask(L, 3, 0.5))),
    ("set_defects_sparse", "set_defects", _sparse),
    ("set_prev_state_array", "set_prev_state_array", lambda e: e.set_prev_state(lo.state_field(L, 4, fill=0.01))),
    ("set_prev_state_null", "set_prev_state_null", lambda e: e.set_prev_state(None)),
    ("apply", "apply", _apply),
    ("thermal_cet", "thermal_update", lambda e: e.thermal_cet(lo.THERMAL_DT, scrub_nan=True)),
    ("thermal_laser", "thermal_update", _laser),
    ("stage_inputs", "batch_begin", lambda e: e.stage_inputs(**_batch(N_STAGED + 1))),
    ("download", None, lambda e: e.download(defects=True)),
]


@pytest.mark.parametrize("n_slabs", [1, 2])
@pytest.mark.parametrize("case,cause,call", CASES, ids=[c[0] for c in CASES])
def test_cause_invalidates_exactly_its_row(case, cause, call, n_slabs):
    _check(case, cause, call, n_slabs)


# ---- remelting, sub-stepped updates, the timers, the maps ------------------------------------------------------------------------
MELT_AT = lo.T_MELT + 0.3          # about half of the deposition plane i = L - 1 of lo.fields lies above it


def _remelt(e):
    assert e.remelt(MELT_AT)["n_melted_last"] > 0, "the pass melts nothing: the case would not show what a melt makes stale"


def _remelt_nothing(e):
    info = e.remelt(float("inf"))
    assert (info["passes"], info["n_melted"]) == (1, 0)


def _time_remelt(e):
    e.time_remelt(2, MELT_AT)
    info = e.remelt_info()
    assert info["passes"] == 3 and info["n_melted"] > 0 and info["n_melted_last"] == 0      # two timed passes, one untimed (cetkmc.h)


def _set_remelt_on_and_off(e):
    e.set_remelt(True, MELT_AT)
    e.set_remelt(False, MELT_AT)


def _set_substeps(e):
    e.set_thermal_substeps(5)
    e.set_thermal_substeps(1)


def _substepped_cet(e):
    e.set_thermal_substeps(5)
    e.set_option("substep_block", 3)
    e.thermal_cet(lo.THERMAL_DT, scrub_nan=True)
    assert e.substep_info()["substeps"] == 5


def _solid_cycle(e):
    e.solid_begin()
    try:
        e.solid_update(1, lo.THERMAL_DT)
        e.solid_read()
    finally:
        e.solid_end()


def _origin_cycle(e):
    e.origin_begin()
    try:
        e.origin_read()
    finally:
        e.origin_end()


# (case, cause or None, the call, on two slabs: "refused" = the call must be refused, "may" = it may be; either way every cache
# must then have survived)
CASES2 = [
    ("remelt", "apply", _remelt, "refused"),
    ("remelt_nothing", "apply", _remelt_nothing, "refused"),        # as the code does: the pass ran, its cause is raised
    ("time_remelt", "apply", _time_remelt, "refused"),
    ("set_remelt_on", None, lambda e: e.set_remelt(True, MELT_AT), "refused"),
    ("set_remelt_on_and_off", None, _set_remelt_on_and_off, "refused"),
    ("set_thermal_substeps_5", None, lambda e: e.set_thermal_substeps(5), None),
    ("set_thermal_substeps_5_and_1", None, _set_substeps, None),
    ("opt_substep_block", None, _option("substep_block", 3), None),
    ("opt_substep_planes", None, _option("substep_planes", 8), None),
    ("thermal_cet_n5_block3", "thermal_update", _substepped_cet, None),
    ("time_thermal", "thermal_update", lambda e: e.time_thermal(2), None),
    ("time_thermal_laser", "thermal_update", lambda e: e.time_thermal(2, laser=True), None),
    ("time_sweeps", None, lambda e: e.time_sweeps(3), None),
    ("event_overhead", None, lambda e: e.event_overhead(5), None),
    ("solid_cycle", None, _solid_cycle, "may"),
    ("origin_cycle", None, _origin_cycle, "may"),
]


@pytest.mark.parametrize("n_slabs", [1, 2])
@pytest.mark.parametrize("case,cause,call,two_slabs", CASES2, ids=[c[0] for c in CASES2])
def test_new_cause_invalidates_exactly_its_row(case, cause, call, two_slabs, n_slabs):
    _check(case, cause, call, n_slabs, two_slabs if n_slabs > 1 else None)


def _check(case, cause, call, n_slabs, refusal=None):
    import cetkmc
    stale = TABLE[cause] if cause else 0
    e = cetkmc.Engine(L, impurity_c=lo.IMPURITY_C, n_slabs=n_slabs)
    try:
        for k, v in dict(lo.BASE_PARAMS, **lo.FIXED_PARAMS).items():
            setattr(e.params, k, v)
        e.set_params()
        e.upload(*_fields(0))
        e.set_option("interface_every_step", 0)
        e.stage_inputs(**_batch(N_STAGED))
        e.rate_sweep()                           # every cache fresh
        e.row_sums()
        before = e.counters()
        e.rate_sweep()
        warm = e.counters()
        assert (warm["table_updates"], warm["interface_launches"]) == (before["table_updates"], before["interface_launches"]), "not warm"

        if refusal is None:
            call(e)
        else:
            try:
                call(e)
                assert refusal == "may", (case, "not refused on a handle with several slabs")
            except RuntimeError as ex:
                assert "in one slab" in str(ex), (case, str(ex))
                stale = 0          # refused before anything was launched: every cache survived

        c0 = e.counters()
        try:
            e.row_sums()
            refused = False
        except RuntimeError as ex:
            assert "cetkmc_row_sums needs a preceding cetkmc_rate_sweep" in str(ex)
            refused = True
        e.rate_sweep()
        c1 = e.counters()
        d_table, d_ifc = c1["table_updates"] - c0["table_updates"], c1["interface_launches"] - c0["interface_launches"]
        try:
            e.run_steps(staged=True, **_batch(N_STAGED))
            survived = True
        except RuntimeError as ex:
            assert "staged batch" in str(ex)
            survived = False
        print(f"{case} slabs={n_slabs}: row_sums refused {refused}, table_updates +{d_table}, interface_launches +{d_ifc}, "
              f"staged batch survived {survived}; row {stale:#x}")
        assert refused == bool(stale & SWEEP), (case, "SWEEP")
        assert d_table == int(bool(stale & TABLE_)), (case, "TABLE")
        assert d_ifc == int(bool(stale & (TABLE_ | IFC))), (case, "IFC")
        assert survived == (not stale & STAGED), (case, "STAGED")
    finally:
        e.close()
