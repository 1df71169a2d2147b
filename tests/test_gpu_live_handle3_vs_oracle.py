"""One LIVE handle through the entry points of the implicit scheme, the thermal boundaries, the beam tables, the shifts and the
lane and tile options, against the oracle after every operation (the third vocabulary, live_ops3.py).

The per-feature tests build a fresh handle, set their switches once and run.  Here ONE handle keeps stepping while the scheme
goes explicit -> implicit -> explicit, boundaries and beams come and go, r and beta of the device's coefficient tables change
under it, the lattice is shifted between calls, a batch that stopped ON an update step is continued behind each of them, and
every documented refusal is walked THROUGH (the refused call must have changed nothing).  After every mutator, setting, option,
read-only and refused call: all five fields and the sweep (helpers.assert_fields_match_oracle); after every stepping call the
whole result; T compares exactly (NaN against NaN), rates and sums within RATE_RTOL.  cetkmc_get_implicit_info, the boundary and
beam records (with both coeff_uploads and table_uploads), cetkmc_remelt_info, cetkmc_substep_info and the shift calls are
compared with what the Runner predicts from the script behind every stepping call and every direct update; at L = 136
cetkmc_lane_table's ``fresh`` after every operation.  tests/test_live_ops3_host.py asserts on the oracle alone that the scripts
cover what they claim."""
import os

import pytest

import live_ops as lo
import live_ops3 as l3
from helpers import assert_call_matches_oracle, assert_fields_match_oracle, assert_local_matches_ref, assert_supersteps_match_oracle
from test_gpu_parity import RATE_RTOL

pytestmark = pytest.mark.gpu

CASES3 = [(16, 1, n) for n in l3.script_names3(16)] + [(24, 1, n) for n in ("walk3", "toggles3")] + [(24, 3, "refusals3")]


def _play3(oracle_mod, L, n_slabs, name, paths=None):
    import cetkmc
    script = l3.make_script3(L, name)
    e = cetkmc.Engine(L, impurity_c=lo.IMPURITY_C, n_slabs=n_slabs)
    try:
        r = l3.Runner3(oracle_mod, L, paths=paths, engine=e, n_slabs=n_slabs,
                       check_fields=lambda e, lat, tag: assert_fields_match_oracle(e, lat, RATE_RTOL, tag),
                       check_run=lambda e, lat, rg, ro, tag: assert_call_matches_oracle(e, lat, rg, ro, RATE_RTOL, tag),
                       check_super=lambda e, lat, rg, ro, tag: assert_supersteps_match_oracle(e, lat, rg, ro, RATE_RTOL, tag),
                       check_local=lambda e, lat, rg, ro, tag: assert_local_matches_ref(e, lat, rg, ro, RATE_RTOL, tag))
        results = []
        for op, tag in zip(script, lo.tags(script, f"L={L} slabs={n_slabs} {name}")):
            results.append((op, tag, r.do(op, tag)))
        r.tag = "the end of the script"
        r._verify_info()
        return r, results, e.counters(), e.substep_info(), e.lane_table()
    finally:
        e.close()


@pytest.mark.parametrize("L,n_slabs,name", CASES3, ids=[f"L{L}-slabs{s}-{n}" for L, s, n in CASES3])
def test_live_handle_third_vocabulary_vs_oracle(oracle_mod, L, n_slabs, name):
    r, results, cnt, sub, lanes = _play3(oracle_mod, L, n_slabs, name)
    for op, tag, ro in results:
        if ro is None:
            continue
        want = ((20, 2) if "cut" in op else (r.paths[op["name"]]["n"] - 20, 0)) if name == "stopped3" else (r.paths[op["name"]]["n"], 0)
        assert (ro["done"], ro["status"]) == want, tag
    assert cnt["deferred_steps"] + r.deferred_reset == r.deferred_expected, (cnt["deferred_steps"], r.deferred_reset, r.deferred_expected)
    assert lanes["chunks"] == 0                       # these shapes have no lane table
    if name == "toggles3":
        assert r.imp["coeff_uploads"] >= 1 and r.bci["coeff_uploads"] >= 4 and r.beami["table_uploads"] >= 3, (r.imp, r.bci, r.beami)
    if name != "refusals3":
        assert r.imp["updates"] > 0 and r.shift_calls > 0, (r.imp, r.shift_calls)
    else:
        assert sub["blocked_launches"] == 0, sub       # several in-process slabs always take the plain path
        assert r.imp["updates"] == r.bci["updates"] == r.beami["updates"] == r.beami["table_uploads"] == r.shift_calls == 0
        assert {f for _, f in r.refusals} >= {lo.REFUSED_SLABS, l3.REFUSED_BOUNDARY_EXPLICIT, l3.REFUSED_BEAM_EXPLICIT, l3.REFUSED_NO_BEAM}


def test_live_handle_third_vocabulary_deferred_path_vs_oracle(oracle_mod):
    """L = 136, the smallest multiple of 8 that defers and has a lane table: every new setting, mutator and option once ahead of
    the deferring call or the same with apply_in_sweep off, then Mode B box 8 and the local loop (which write table entries
    through ifc_store()) alternating with the deferring call, and a shift.  cetkmc_lane_table is compared after every operation:
    ``fresh`` with the invalidation rules before the next plain launch, the builds of that launch, and the builds of every
    deferring call."""
    L = 136
    oracle_mod.set_threads(min(16, os.cpu_count() or 1))
    try:
        r, results, cnt, sub, lanes = _play3(oracle_mod, L, 1, "pairs3_deferred", paths=lo.deferred_paths())
    finally:
        oracle_mod.set_threads(1)
    for op, tag, ro in results:
        if ro is not None:
            assert (ro["done"], ro["status"]) == (r.paths[op["name"]]["n"], 0), tag
    assert cnt["deferred_steps"] == r.deferred_expected > 20, (cnt["deferred_steps"], r.deferred_expected)
    assert cnt["incremental_steps"] == 0
    # every build is accounted for: those of a comparison's plain launch and of the deferring calls are predicted one by one
    # (Runner3._verify, Runner3.step), those of the Mode B and local calls are read; + 1: the upload's sweep at creation
    assert lanes["chunks"] > 0 and r.lane_checks > 40 and r.lane_call_checks > 25, (lanes, r.lane_checks, r.lane_call_checks)
    assert lanes["builds"] + lanes["builds_thermal"] == r.lane_builds + r.lane_builds0 > 10, (lanes, r.lane_builds, r.lane_builds0)
    assert r.imp["updates"] > 0 and r.bci["updates"] > 0 and r.beami["updates"] > 0 and r.shift_calls == 4, (r.imp, r.bci, r.beami, r.shift_calls)
