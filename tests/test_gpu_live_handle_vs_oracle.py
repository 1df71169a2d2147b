"""One LIVE handle through every mutating entry point between steps, against the oracle after every operation.

The host layer of the library is a cache state machine: about fifteen entry points change the lattice
or its parameters and each resets its own subset of the freshness flags.  A forgotten reset leaves the next sweep reading a
stale rate table, stale interface sums or a stale list -- a plausible, wrong trajectory and no fault.  The scripts of
live_ops.py put every mutator M ahead of every stepping path S on a handle whose caches a previous call of S has just made
fresh (``pairs``), walk at random over mutators, read-only calls and paths (``walk``), alternate Mode A and Mode B with
growing and shrinking box counts (``modes``) and step on behind a termination (``frozen``).  After every mutator and
read-only call: all five fields and the sweep of the lattice (helpers.assert_fields_match_oracle); after every stepping call
the whole result.  Integers, positions and fields compare with ==, rates and sums within RATE_RTOL.
tests/test_live_ops_host.py asserts on the oracle alone that the scripts cover what they claim.  The entry points of remelting,
sub-stepped temperature updates, the local Mode B loop and the timers have scripts of their own at the end of this file.

Pinned as the code does it today (include/cetkmc.h): the nucleation count and cetkmc_counters survive an upload of a whole
new lattice; a staged batch survives every mutator and then steps the mutated lattice."""
import os

import pytest

import live_ops as lo
from helpers import assert_call_matches_oracle, assert_fields_match_oracle, assert_local_matches_ref, assert_supersteps_match_oracle
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

CASES = [(L, n_slabs, name) for L, n_slabs in ((16, 1), (24, 3)) for name in lo.script_names(L)]


def _play(oracle_mod, L, n_slabs, name, paths=None):
    import cetkmc
    script = lo.make_script(L, name)
    e = cetkmc.Engine(L, impurity_c=lo.IMPURITY_C, n_slabs=n_slabs)
    try:
        r = lo.Runner(oracle_mod, L, paths=paths, engine=e, n_slabs=n_slabs,
                      check_fields=lambda e, lat, tag: assert_fields_match_oracle(e, lat, RATE_RTOL, tag),
                      check_run=lambda e, lat, rg, ro, tag: assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, tag),
                      check_super=lambda e, lat, rg, ro, tag: assert_supersteps_match_oracle(e, lat, rg, ro, RATE_RTOL, tag))
        results = []
        for op, tag in zip(script, lo.tags(script, f"L={L} slabs={n_slabs} {name}")):
            results.append((op, tag, r.do(op, tag)))
        return r, results, e.counters()
    finally:
        e.close()


@pytest.mark.parametrize("L,n_slabs,name", CASES, ids=[f"L{L}-slabs{s}-{n}" for L, s, n in CASES])
def test_live_handle_vs_oracle(oracle_mod, L, n_slabs, name):
    r, results, cnt = _play(oracle_mod, L, n_slabs, name)
    for op, tag, ro in results:
        if ro is None:
            continue
        if name != "frozen":          # (the engine's done / status equal the oracle's: asserted by the comparison)
            assert (ro["done"], ro["status"]) == (r.paths[op["name"]]["n"], 0), tag
        elif op["expect"] == "unfrozen":
            assert ro["done"] > 0, tag
        else:
            assert ro["status"] == 1 and (ro["done"] == 0) == (op["expect"] == "stays_frozen"), tag
    assert cnt["deferred_steps"] + r.deferred_reset == r.deferred_expected, (cnt["deferred_steps"], r.deferred_reset, r.deferred_expected)


def test_live_handle_deferred_path_vs_oracle(oracle_mod):
    """L = 136, the smallest multiple of 8 on the deferring path: every mutator once ahead of the default (deferring) batched
    call or the same with apply_in_sweep off; cetkmc_counters.deferred_steps proves which steps were deferred."""
    L = 136
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        r, results, cnt = _play(oracle_mod, L, 1, "pairs_deferred", paths=lo.deferred_paths())
    finally:
        oracle_mod.set_threads(1)
    for op, tag, ro in results:
        if ro is not None:
            assert (ro["done"], ro["status"]) == (r.paths[op["name"]]["n"], 0), tag
    assert cnt["deferred_steps"] == r.deferred_expected > 20, (cnt["deferred_steps"], r.deferred_expected)
    assert cnt["incremental_steps"] == 0


def test_staged_batch_is_consumed_once_and_dropped_by_buffer_moves(oracle_mod):
    """The rule of cetkmc_stage_inputs: one cetkmc_run_steps consumes the batch; a second one without inputs, and one behind
    a call that reuses or moves the batch buffers (run_supersteps, reserve_batch), are refused and change nothing."""
    import cetkmc
    L = 16
    e = cetkmc.Engine(L, impurity_c=lo.IMPURITY_C)
    try:
        r = lo.Runner(oracle_mod, L, engine=e, check_fields=lambda e, lat, tag: assert_fields_match_oracle(e, lat, RATE_RTOL, tag),
                      check_run=lambda e, lat, rg, ro, tag: assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, tag),
                      check_super=lambda e, lat, rg, ro, tag: assert_supersteps_match_oracle(e, lat, rg, ro, RATE_RTOL, tag))
        pname = "a_rng1_full_laser_none"
        spec = r.paths[pname]
        inp = lo.step_inputs(L, spec, 3)
        kw = dict(rng_mode=spec["rng_mode"], seed=lo.COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=lo.THERMAL_DT)

        def run_staged():
            return e.run_steps(spec["step0"], spec["n"], lo.DEFECT_FRACTION, None, None, None, q_planes=None, staged=True, **kw)

        r.do(dict(kind="mut", name="staged", seed=1, path=pname, step_seed=3), "stage, mutate")
        r.do(dict(kind="step", name=pname, seed=3, staged=True), "consume the staged batch")
        for what, drop in (("consumed", lambda: None), ("run_supersteps", lambda: r.do(dict(kind="step", name="b_box8", seed=4, staged=False), "Mode B")),
                           ("reserve_batch", lambda: r.do(dict(kind="opt", name="opt_reserve_batch=4096"), "reserve"))):
            if what != "consumed":
                e.stage_inputs(spec["step0"], spec["n"], lo.DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"], q_planes=inp["q"], **kw)
            drop()
            with pytest.raises(RuntimeError, match="no staged batch"):
                run_staged()
            assert_fields_match_oracle(e, r.lat, RATE_RTOL, f"refused staged run behind {what}")
        # a staged batch of another shape is refused as well, and the right call still finds it afterwards? No: refusing drops it
        e.stage_inputs(spec["step0"], spec["n"], lo.DEFECT_FRACTION, inp["u_pick"], inp["u_def"], inp["u_np"], q_planes=inp["q"], **kw)
        with pytest.raises(RuntimeError, match="does not match"):
            e.run_steps(spec["step0"] + 1, spec["n"], lo.DEFECT_FRACTION, None, None, None, staged=True, **kw)
        with pytest.raises(RuntimeError, match="no staged batch"):
            run_staged()
        assert_fields_match_oracle(e, r.lat, RATE_RTOL, "refused staged runs")
        assert e.nucleation_count() == r.lat.nuc_count
    finally:
        e.close()


# ---- the second vocabulary: remelting, sub-stepped updates, the local Mode B loop, the timers (live_ops.py) ------------------------
CASES2 = [(L, n_slabs, name) for L, n_slabs in ((16, 1), (24, 3)) for name in lo.script_names2(L)]


def _play2(oracle_mod, L, n_slabs, name, paths=None):
    import cetkmc
    script = lo.make_script(L, name)
    e = cetkmc.Engine(L, impurity_c=lo.IMPURITY_C, n_slabs=n_slabs)
    try:
        r = lo.Runner(oracle_mod, L, paths=paths, engine=e, n_slabs=n_slabs,
                      check_fields=lambda e, lat, tag: assert_fields_match_oracle(e, lat, RATE_RTOL, tag),
                      check_run=lambda e, lat, rg, ro, tag: assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, tag),
                      check_super=lambda e, lat, rg, ro, tag: assert_supersteps_match_oracle(e, lat, rg, ro, RATE_RTOL, tag),
                      check_local=lambda e, lat, rg, ro, tag: assert_local_matches_ref(e, lat, rg, ro, RATE_RTOL, tag))
        results = []
        for op, tag in zip(script, lo.tags(script, f"L={L} slabs={n_slabs} {name}")):
            results.append((op, tag, r.do(op, tag)))
        return r, results, e.counters(), e.substep_info()
    finally:
        e.close()


@pytest.mark.parametrize("L,n_slabs,name", CASES2, ids=[f"L{L}-slabs{s}-{n}" for L, s, n in CASES2])
def test_live_handle_second_vocabulary_vs_oracle(oracle_mod, L, n_slabs, name):
    """The scripts over remelting, sub-stepped updates, the local loop and the timers.  T behind the sub-stepped updates compares
    bit for bit (NaN against NaN) with the rest of the fields; cetkmc_remelt_info and cetkmc_substep_info are compared behind
    every stepping call and every direct pass (Runner._verify_info); a refused call must have changed nothing."""
    r, results, cnt, sub = _play2(oracle_mod, L, n_slabs, name)
    for op, tag, ro in results:
        if ro is None:
            continue
        want = ((20, 2) if "cut" in op else (r.paths[op["name"]]["n"] - 20, 0)) if name == "stopped" else (r.paths[op["name"]]["n"], 0)
        assert (ro["done"], ro["status"]) == want, tag
    assert cnt["deferred_steps"] + r.deferred_reset == r.deferred_expected, (cnt["deferred_steps"], r.deferred_reset, r.deferred_expected)
    if n_slabs == 1 and name.startswith("pairs2:a_") and r.sub["updates"]:
        # block 3 with 8 planes per block on a one-slab handle: the temporally blocked kernel ran (at L = 24 in three plane groups)
        assert sub["blocked_launches"] > 0, sub
    if n_slabs > 1:
        assert sub["blocked_launches"] == 0, sub          # several in-process slabs always take the plain path
        assert lo.REFUSED_SLABS in {f for _, f in r.refusals} or not any(op["name"].startswith(("remelt", "time_remelt", "set_remelt", "local"))
                                                                         for op, _, _ in results)


def test_live_handle_second_vocabulary_deferred_path_vs_oracle(oracle_mod):
    """L = 136 on the deferring path: every new mutator, setting and option once.  With n = 5 and no option set the update takes
    the default dispatch of the temporally blocked kernel (three sub-steps, then the remainder): blocked_launches proves it."""
    L = 136
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        r, results, cnt, sub = _play2(oracle_mod, L, 1, "pairs2_deferred", paths=lo.deferred_paths())
    finally:
        oracle_mod.set_threads(1)
    for op, tag, ro in results:
        if ro is not None:
            assert (ro["done"], ro["status"]) == (r.paths[op["name"]]["n"], 0), tag
    assert cnt["deferred_steps"] == r.deferred_expected > 5, (cnt["deferred_steps"], r.deferred_expected)
    assert cnt["incremental_steps"] == 0
    assert sub["blocked_launches"] > 0 and sub["updates"] == r.sub["updates"] > 0, (sub, r.sub)
