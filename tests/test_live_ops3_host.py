"""The scripts of live_ops3.py on the oracle alone: the conditions that keep tests/test_gpu_live_handle3_vs_oracle.py from
passing vacuously.  Everything of the third vocabulary occurs, every (M, S) pair occurs, the documented refusals are met,
stepping calls run to their end, all four event kinds fire (nucleation and diffusion right behind every new class), the call
behind a shift executes an event at the seam, every setting changes the field of the next update and every no-op changes
nothing, the coefficient tables are rebuilt for beta, n and dt alone, and no pick hangs on the last bits of a total."""
import hashlib

import numpy as np
import pytest

import live_ops as lo
import live_ops3 as l3
from shift_cases import events_in_zone

CASES = [(16, 1, n) for n in l3.script_names3(16)] + [(24, 1, n) for n in ("walk3", "toggles3")] + [(24, 3, "refusals3")]
NEW_CLASSES = set(l3.MUTATORS3.values())


def _class_of(op):
    n = op["name"]
    return (l3.MUTATORS3.get(n) or lo.MUTATORS2.get(n) or lo.MUTATORS.get(n) or
            ("options" if n.startswith("opt_") else "read_only" if op["kind"] == "ro" else n))


def _settings_of(r):
    return (r.implicit, r.bc_name, r.beam_name)


def _next_update(oracle_mod, r, settings):
    """the field after one laser update of ordinal 1 with ``settings`` = (implicit, boundary, beam), on a clone"""
    import beam_ref
    import boundary_ref
    from cetkmc import synthetic
    c = lo.clone(oracle_mod, r.lat)
    implicit, bc, beam = settings
    q = synthetic.laser_planes(r.L, 20, 1, power=lo.LASER_POWER)[0]
    if not implicit:
        c.thermal_laser(lo.THERMAL_DT, q, scrub_nan=True, update_prev=True)
    elif beam is not None:
        beam_ref.update(c, 1, lo.THERMAL_DT, l3.beam_table(r.L, beam), 1, bc=l3.boundary_of(bc))
    else:
        boundary_ref.update(c, 1, lo.THERMAL_DT, 2, q, bc=l3.boundary_of(bc), u=1)
    return c.T


def _play3(oracle_mod, L, n_slabs, name):
    script = l3.make_script3(L, name)
    r = l3.Runner3(oracle_mod, L, n_slabs=n_slabs, paths=lo.deferred_paths() if L > 128 else None)
    recs, shifted = [], None
    for op, tag in zip(script, lo.tags(script, f"L={L} {name}")):
        rec = dict(op=op, tag=tag, settings=_settings_of(r))
        n_ref = len(r.refusals)
        if op["kind"] == "step":
            spec = r.paths[op["name"]]
            before, marker = lo.clone(oracle_mod, r.lat), r.marker
            n_sub, thr = r.substeps, r.remelt_threshold if r.remelt_on else None
            ro = r.do(op, tag)
            rec.update(ro=ro, spec=spec, refused=len(r.refusals) > n_ref, last=dict(r.last))
            if ro is not None:
                rec["kinds"] = lo.event_kinds(spec, ro)
                if shifted is not None:
                    rec["in_zone"] = events_in_zone(L, shifted, np.asarray(ro["events"]) if spec["kind"] != "loop" else
                                                    np.array([(e[0], e[1], e[2]) for e in ro["events"]],
                                                             dtype=[("type", "<i4"), ("pos", "<i4", 3), ("target", "<i4", 3)]))
                    shifted = None
                if spec["kind"] == "loop" or (spec["kind"] == "run" and spec["rng_mode"] != 2):
                    inp = r.last.get("inp") or lo.step_inputs(L, spec, op["seed"])
                    step0, n = r.last.get("args", (spec.get("step0"), spec["n"]))
                    for scale in (1 - 1e-9, 1 + 1e-9):
                        c = lo.clone(oracle_mod, before)
                        if "inp" in r.last:
                            st = l3.make_stepper(c, rec["settings"][0], n_sub, thr, l3.boundary_of(rec["settings"][1]),
                                                 None if rec["settings"][2] is None else l3.beam_table(L, rec["settings"][2]))
                            st.applied_g = marker
                            rp = st.run_steps(step0, n, lo.DEFECT_FRACTION, inp["u_pick"] * scale, inp["u_def"], inp["u_np"],
                                              rng_mode=spec["rng_mode"], seed=lo.COUNTER_SEED, thermal_mode=spec["thermal_mode"],
                                              thermal_dt=lo.THERMAL_DT, q_planes=inp["q"])
                        else:
                            rp = lo.oracle_step(c, spec, inp, scale)
                        assert lo.event_key(spec, rp) == lo.event_key(spec, ro), f"{tag}: a pick flips with u_pick * {scale!r}: pick another seed"
        else:
            cls = _class_of(op)
            sig = "impurity" if op["name"] == "param_impurity_c" else "thermal" if cls in ("shift", "shift_noop", "beam_update") else cls
            sig_before = lo.mutator_signature(oracle_mod, r.lat, sig)
            r.do(op, tag)
            refused = len(r.refusals) > n_ref
            rec.update(cls=cls, refused=refused, last=dict(r.last), changed=lo.mutator_signature(oracle_mod, r.lat, sig) != sig_before)
            if cls == "setting3" and not refused and _settings_of(r) != rec["settings"]:
                a, b = _next_update(oracle_mod, r, rec["settings"]), _next_update(oracle_mod, r, _settings_of(r))
                rec["update_differs"] = int((a.view(np.int64) != b.view(np.int64)).sum())
            if cls == "shift" and not refused:
                shifted = l3.SHIFTS[op["name"]]["d"]
        recs.append(rec)
    return recs, r


@pytest.fixture(scope="module")
def played3(oracle_mod):
    return {(L, s, n): _play3(oracle_mod, L, s, n) for L, s, n in CASES}


def _steps(recs):
    return [r for r in recs if r["op"]["kind"] == "step"]


def test_third_vocabulary_occurs(played3):
    for L in (16, 24):
        recs, _ = played3[(L, 1, "walk3")]
        seen = [r["op"]["name"] for r in recs]
        everything = (set(lo.MUTATORS) | set(lo.MUTATORS2) | set(l3.MUTATORS3) | set(lo.READ_ONLY) | set(lo.READ_ONLY2) | set(l3.READ_ONLY3) |
                      set(l3.paths3(L)))
        for x in everything:
            assert seen.count(x) >= 2, (L, "walk3", x, seen.count(x))
        assert len(seen) >= 250, len(seen)
        since = 0
        for rec in recs:             # a stepping call at least every third operation of those the walk drew
            since = 0 if rec["op"]["kind"] == "step" else since + 1
            assert since <= 8, rec["tag"]
    for p in l3.mode_a_paths(16):    # pairs3: every M directly ahead of a call of S, which a call of S precedes
        names = [r["op"]["name"] for r in played3[(16, 1, f"pairs3:{p}")][0]]
        assert [n for n in names if not n.startswith("param_")][0] == p
        for m in list(l3.MUTATORS3) + list(l3.IMPLICIT_TOO):
            hits = [q for q, x in enumerate(names) if x == m and names[q + 1:q + 2] == [p] and p in names[:q]]
            assert hits, (p, m)
    assert {lo.stepping_paths(16)[p]["kind"] for p in l3.mode_a_paths(16)} == {"run", "loop"}


def test_implicit_mutators_are_met_while_the_scheme_is_implicit(played3):
    for p in l3.mode_a_paths(16):
        recs, _ = played3[(16, 1, f"pairs3:{p}")]
        for m in l3.IMPLICIT_TOO:
            assert any(r["op"]["name"] == m and r["settings"][0] and not r["refused"] for r in recs if r["op"]["kind"] != "step"), (p, m)


def test_refusals_are_met(played3):
    one_slab = set()
    for L in (16, 24):
        for name in ("walk3", "toggles3"):
            if (L, 1, name) in played3:
                one_slab |= {f for _, f in played3[(L, 1, name)][1].refusals}
    want = {l3.REFUSED_IMPLICIT, lo.REFUSED_LOOKAHEAD, l3.REFUSED_BOUNDARY_SET, l3.REFUSED_BEAM_SET, l3.REFUSED_BOUNDARY_EXPLICIT,
            l3.REFUSED_BEAM_EXPLICIT, l3.REFUSED_LASER_BEAM, l3.REFUSED_PLANES_BEAM, l3.REFUSED_STEP_ROWS, l3.REFUSED_BEAM_ROW}
    assert want <= one_slab, want - one_slab
    # keyed by the refused operation: Mode B, the local loop and thermal_lookahead = 1 against the implicit scheme, the
    # implicit scheme against the look-ahead, and the rest of the list -- each of them met in walk3 or toggles3
    met = set()
    for L in (16, 24):
        for name in ("walk3", "toggles3"):
            recs, r = played3[(L, 1, name)]
            frags = iter(r.refusals)
            for rec in recs:
                if rec["refused"]:
                    name = rec["op"]["name"]
                    what = (rec["spec"]["kind"] if rec["op"]["kind"] == "step" else
                            name[:12] if name.startswith("set_boundary_") else name[:8] if name.startswith("set_beam_") else name)
                    met.add((what, next(frags)[1]))
    want = {("super", l3.REFUSED_IMPLICIT), ("local", l3.REFUSED_IMPLICIT), ("opt_thermal_lookahead=1", l3.REFUSED_IMPLICIT),
            ("set_scheme_implicit", lo.REFUSED_LOOKAHEAD), ("set_scheme_explicit", l3.REFUSED_BOUNDARY_SET),
            ("set_scheme_explicit", l3.REFUSED_BEAM_SET), ("set_boundary", l3.REFUSED_BOUNDARY_EXPLICIT), ("set_beam", l3.REFUSED_BEAM_EXPLICIT),
            ("thermal_laser", l3.REFUSED_LASER_BEAM), ("run", l3.REFUSED_PLANES_BEAM), ("run", l3.REFUSED_STEP_ROWS),
            ("thermal_beam", l3.REFUSED_BEAM_ROW)}
    assert want <= met, want - met
    recs, r = played3[(24, 3, "refusals3")]
    refused = {rec["op"]["name"] for rec in recs if rec["refused"] and rec["op"]["kind"] != "step"}
    assert set(l3.REFUSED_ON_SLABS) <= refused, set(l3.REFUSED_ON_SLABS) - refused
    assert _settings_of(r) == (False, None, None) and r.imp["updates"] == r.bci["updates"] == r.beami["updates"] == r.shift_calls == 0
    assert {"run", "loop", "super", "local"} == {rec["spec"]["kind"] for rec in _steps(recs)}


def test_stepping_calls_run_to_their_end(played3):
    for (L, s, name), (recs, _) in played3.items():
        for rec in _steps(recs):
            if rec["refused"]:
                assert rec["ro"] is None, rec["tag"]
            elif name != "stopped3":
                assert (rec["ro"]["done"], rec["ro"]["status"]) == (rec["spec"]["n"], 0), rec["tag"]
    recs, _ = played3[(16, 1, "stopped3")]
    steps = _steps(recs)
    between = [rec["op"]["name"] for q, rec in enumerate(recs) if 0 < q and "cut" in recs[q - 1]["op"]]
    assert between == [x for _, x, _ in l3.STOPPED3_KEEP + l3.STOPPED3_DROP]
    assert len(steps) == 2 * len(between)
    for first, second in zip(steps[0::2], steps[1::2]):
        assert (first["ro"]["done"], first["ro"]["status"]) == (20, 2), first["tag"]
        assert (second["ro"]["done"], second["ro"]["status"]) == (first["spec"]["n"] - 20, 0), second["tag"]
        assert second["last"]["marker"] == (20 if second["op"]["keeps"] else -1), second["tag"]
        if second["last"]["beam"] is not None:
            assert second["last"]["inp"]["q"] is None, second["tag"]          # with a beam set the continuation needs no plane
    assert sum(s["op"].get("keeps", False) for s in steps) == len(l3.STOPPED3_KEEP)


def test_all_four_kinds_fire(played3):
    pairs = np.zeros(4, np.int64)
    for (L, s, name), (recs, _) in played3.items():
        k = sum(rec["kinds"] for rec in _steps(recs) if not rec["refused"])
        if name.startswith("pairs3:"):
            pairs += k
        assert k.min() >= 1, (L, name, k)
    assert pairs.min() >= 20, pairs


def test_nucleation_and_diffusion_right_behind_every_new_class(played3):
    first = {}
    for (L, s, name), (recs, _) in played3.items():
        if not (name.startswith("pairs3:") or name == "walk3"):
            continue
        script = "pairs3" if name.startswith("pairs3:") else (name, L)
        pending = set()
        for rec in recs:
            if rec["op"]["kind"] == "step":
                if not rec["refused"]:
                    for cls in pending:
                        first.setdefault((script, cls), np.zeros(4, np.int64))
                        first[(script, cls)] += rec["kinds"]
                    pending = set()
            elif not rec["refused"] and rec["cls"] in NEW_CLASSES:
                pending.add(rec["cls"])
    for script in ("pairs3", ("walk3", 16), ("walk3", 24)):
        for cls in NEW_CLASSES:
            k = first[(script, cls)]
            assert k[1] >= 1 and k[2] >= 1, (script, cls, k)


def test_an_event_at_the_seam_behind_every_shift(played3):
    n = 0
    for (L, s, name), (recs, _) in played3.items():
        for rec in _steps(recs):
            if "in_zone" in rec:
                n += 1
                assert rec["in_zone"] >= 1, rec["tag"]
    assert n >= 30


def test_settings_change_the_next_update_and_no_ops_change_nothing(played3):
    seen = set()
    for (L, s, name), (recs, _) in played3.items():
        for rec in recs:
            if rec["op"]["kind"] == "step" or rec["refused"]:
                continue
            if rec["cls"] in l3.NOOP_CLASSES3 or rec["cls"] == "read_only":
                assert not rec["changed"], rec["tag"]
            else:
                assert rec["changed"], rec["tag"]
            if "update_differs" in rec:
                seen.add(rec["op"]["name"])
                assert rec["update_differs"] >= L * L, (rec["tag"], rec["update_differs"])
    assert seen == set(l3.SETTINGS3) - {"set_beam_short"} or seen == set(l3.SETTINGS3), seen


def test_table_changes_are_real(played3):
    for L in (24,):
        recs, r = played3[(L, 1, "toggles3")]
        causes = [c for _, _, c in r.coef_log]
        assert {"beta", "n", "dt"} <= set(causes), r.coef_log
        assert r.beami["table_uploads"] >= 3 and r.imp["coeff_uploads"] >= 1 and r.bci["coeff_uploads"] >= 4, (r.imp, r.bci, r.beami)
        runs = [rec for rec in _steps(recs) if not rec["refused"] and rec["spec"]["kind"] == "run"]
        assert all(rec["spec"]["step0"] in (19, 20, 39) and lo.updates_before(rec["spec"]["step0"], rec["spec"]["n"]) for rec in runs)
        combos = [rec["settings"] + (rec["last"].get("substeps", 1), rec["last"].get("threshold") is not None) for rec in runs]
        for want in ((True, None, None, 1, False), (True, "sink", None, 1, False), (True, "sink", "d1", 1, False), (True, "sink", "d1", 3, False),
                     (True, "sink", "d1", 3, True), (True, "mixed", "d1", 3, True), (True, "mixed", "d1", 1, True), (True, "mixed", "d3", 1, True),
                     (True, "mixed", None, 1, True), (True, None, None, 1, True), (True, None, None, 1, False)):
            assert want in combos, (want, combos)
        assert {"super", "local"} <= {rec["spec"]["kind"] for rec in _steps(recs) if not rec["refused"]}
        assert r.shift_calls == 2


def test_deferred_pairs3_script_shape():
    ops = l3.make_script3(136, "pairs3_deferred")
    names = [op["name"] for op in ops]
    for m in l3.MUTATORS3:
        assert [q for q, x in enumerate(names) if x == m and names[q + 1:q + 2] and names[q + 1] in lo.deferred_paths()], m
    tail = [n for n in names[-7:]]
    assert tail == ["a_deferred", "b_box8", "a_deferred", "local_k4", "a_deferred", "shift_layer", "a_deferred"]
    # the read-only calls at the shape that has a lane table: behind a warm deferring call and behind a stale-making mutator
    ro = [q for q, op in enumerate(ops) if op["kind"] == "ro"]
    assert {names[q] for q in ro} == set(l3.READ_ONLY3)
    for x in ("lane_table", "lane_table_arrays"):
        assert any(names[q] == x and ops[[p for p in range(q) if ops[p]["kind"] != "ro"][-1]]["name"] in lo.deferred_paths() for q in ro), x
        assert any(names[q] == x and ops[[p for p in range(q) if ops[p]["kind"] != "ro"][-1]]["name"] == "set_defects" for q in ro), x


# sha256(repr(make_script3(L, name)))[:16] with the seeds of live_ops3.SCRIPT_SEEDS3
PINNED3 = {
    (16, 'pairs3:a_rng0_full_cet_first'): '37fd73d35d5f3935', (16, 'pairs3:a_rng0_incr_laser_inside'): 'a6edf95d17257f9a',
    (16, 'pairs3:a_rng1_full_laser_none'): '7fd1d91006398434', (16, 'pairs3:a_rng1_incr_cet_first20'): '69cb98d857bc88f3',
    (16, 'pairs3:a_rng1_full_cet_last'): 'caf55a1fd68e1612', (16, 'pairs3:a_rng2_full_nothermal'): '1bb1f8a26e75b622',
    (16, 'pairs3:a_rng2_incr_laser_first'): '5482fd95f921a07d', (16, 'pairs3:loop_single_calls'): 'aabbb7f45fb7cf91',
    (16, 'walk3'): '2fd3e5b85eae44fc', (16, 'toggles3'): '56f0fd29667a61a9',
    (16, 'stopped3'): '3ac41e8b1e180949', (24, 'walk3'): '4b7309f7dcdfea97',
    (24, 'toggles3'): '56f0fd29667a61a9', (24, 'refusals3'): 'e8abf36ba29551a4',
    (136, 'pairs3_deferred'): '857c07dd75a7f4b1',
}


def test_third_vocabulary_scripts_are_pinned():
    got = {(L, n): hashlib.sha256(repr(l3.make_script3(L, n)).encode()).hexdigest()[:16]
           for L, n in [(L, n) for L, _, n in CASES] + [(136, "pairs3_deferred")]}
    assert got == PINNED3, got
