"""The operation scripts of live_ops.py on the oracle alone: the conditions that keep tests/test_gpu_live_handle_vs_oracle.py
from passing vacuously.  Every mutator, read-only call and stepping path occurs; every (mutator, path) pair occurs; stepping
calls run to their end; all four event kinds fire, also right behind every class of mutator; every mutator changes what the
next sweep sees and every documented no-op does not; the frozen script freezes and thaws where it says; and the picks of the
host-stream modes do not hang on the last bits of a total."""
import numpy as np
import pytest

import live_ops as lo

SIZES = (16, 24)


def _play(oracle_mod, L, name, paths=None):
    """Runs script ``name`` on the oracle; returns per-operation records dict(op, tag, ro, kinds, changed)."""
    script = lo.make_script(L, name)
    tags = lo.tags(script, f"L={L} {name}")
    r = lo.Runner(oracle_mod, L, paths=paths)
    recs = []
    for op, tag in zip(script, tags):
        rec = dict(op=op, tag=tag)
        if op["kind"] == "step":
            spec = r.paths[op["name"]]
            inp = lo.step_inputs(L, spec, op["seed"])
            probes = [lo.clone(oracle_mod, r.lat) for _ in range(2)] if spec["kind"] == "loop" or spec.get("rng_mode", 2) != 2 else []
            ro = r.do(op, tag)
            rec.update(ro=ro, spec=spec, kinds=lo.event_kinds(spec, ro))
            for c, scale in zip(probes, (1 - 1e-9, 1 + 1e-9)):
                rp = lo.oracle_step(c, spec, inp, scale)
                assert lo.event_key(spec, rp) == lo.event_key(spec, ro), f"{tag}: a pick flips with u_pick * {scale!r}: pick another seed"
        else:
            cls = lo.MUTATORS.get(op["name"], "options" if op["name"].startswith("opt_") else "read_only" if op["kind"] == "ro" else op["name"])
            sig = "impurity" if op["name"] == "param_impurity_c" else cls
            before = lo.mutator_signature(oracle_mod, r.lat, sig)
            r.do(op, tag)
            rec.update(cls=cls, changed=lo.mutator_signature(oracle_mod, r.lat, sig) != before)
        recs.append(rec)
    return recs


@pytest.fixture(scope="module")
def played(oracle_mod):
    return {(L, n): _play(oracle_mod, L, n) for L in SIZES for n in lo.script_names(L)}


def _steps(recs):
    return [r for r in recs if r["op"]["kind"] == "step"]


def test_everything_occurs(played):
    for L in SIZES:
        paths = set(lo.stepping_paths(L))
        seen = [r["op"]["name"] for r in played[(L, "walk")]]
        assert set(lo.MUTATORS) <= set(seen) and set(lo.READ_ONLY) <= set(seen) and paths <= set(seen), (L, "walk")
        assert 200 <= len(seen) <= 340
        for p in paths:          # pairs: every mutator M directly ahead of a call of S, which a call of S precedes
            recs = played[(L, f"pairs:{p}")]
            names = [r["op"]["name"] for r in recs]
            assert names[0] == p
            for m in lo.MUTATORS:
                q = names.index(m)
                nxt = [n for n in names[q + 1:q + 3] if n in paths]
                assert nxt and nxt[0] == p, (L, p, m, names[q:q + 3])
                assert p in names[:q], (L, p, m)
        assert any(r["spec"]["box"] == 8 for r in _steps(played[(L, "modes")]) if r["spec"]["kind"] == "super")
        assert {"run", "loop", "super"} == {s["kind"] for s in lo.stepping_paths(L).values()}
    assert {"b_box12", "b_box12_null"} <= set(lo.stepping_paths(24))
    # offsets modulo 20 of the batched calls: update first (0 and 20), last, inside, not at all
    runs = [s for s in lo.stepping_paths(24).values() if s["kind"] == "run"]
    assert {s["step0"] for s in runs} >= {0, 1, 19, 20}
    assert {(s["rng_mode"], s["incremental"]) for s in runs} == {(m, i) for m in (0, 1, 2) for i in (False, True)}
    assert {s["thermal_mode"] for s in runs} == {0, 1, 2}


def test_stepping_calls_run_to_their_end(played):
    for (L, name), recs in played.items():
        if name == "frozen":
            continue
        for r in _steps(recs):
            assert (r["ro"]["done"], r["ro"]["status"]) == (r["spec"]["n"], 0), r["tag"]


def test_all_four_kinds_fire(played):
    for L in SIZES:
        pairs = np.zeros(4, np.int64)
        for (l, name), recs in played.items():
            if l != L or name == "frozen":
                continue
            k = sum(r["kinds"] for r in _steps(recs))
            if name.startswith("pairs:"):
                pairs += k
            else:
                assert k.min() >= 2, (L, name, k)
        assert pairs.min() >= 20, (L, "pairs", pairs)


def test_nucleation_and_diffusion_right_behind_every_mutator_class(played):
    for L in SIZES:
        first = {}
        for (l, name), recs in played.items():
            if l != L or not (name.startswith("pairs:") or name == "walk"):
                continue
            script = "pairs" if name.startswith("pairs:") else name
            cls = None
            for r in recs:
                if r["op"]["kind"] == "step":
                    if cls is not None:
                        first.setdefault((script, cls), np.zeros(4, np.int64))
                        first[(script, cls)] += r["kinds"]
                    cls = None
                elif r["op"]["kind"] == "mut":
                    cls = r["cls"]
        for script in ("pairs", "walk"):
            for cls in set(lo.MUTATORS.values()):
                k = first[(script, cls)]
                assert k[1] >= 1 and k[2] >= 1, (L, script, cls, k)


def test_mutators_change_the_next_sweep_and_no_ops_do_not(played):
    for (L, name), recs in played.items():
        for r in recs:
            if r["op"]["kind"] == "step":
                continue
            if r["cls"] in lo.NOOP_CLASSES or r["cls"] == "read_only":
                assert not r["changed"], r["tag"]
            else:
                assert r["changed"], r["tag"]


def test_frozen_script_freezes_and_thaws(played):
    for L in SIZES:
        seen = {"terminates": 0, "stays_frozen": 0, "unfrozen": 0}
        kinds = set()
        for r in _steps(played[(L, "frozen")]):
            ro, want = r["ro"], r["op"]["expect"]
            seen[want] += 1
            kinds.add(r["spec"]["kind"])
            if want == "terminates":
                assert ro["status"] == 1 and 0 < ro["done"] < r["spec"]["n"], (r["tag"], ro["done"], ro["status"])
            elif want == "stays_frozen":
                assert (ro["done"], ro["status"]) == (0, 1), (r["tag"], ro["done"], ro["status"])
                assert ro["totals"][0] == 0.0
            else:
                assert ro["done"] > 0, (r["tag"], ro["done"], ro["status"])
        assert kinds == {"run", "super"} and min(seen.values()) == 2 * len(lo.FROZEN_UNFREEZERS)


def test_deferred_pairs_script_shape():
    """The L > 128 case: every mutator once, both stepping paths, batches of at most 8 steps."""
    ops = lo.make_script(136, "pairs_deferred")
    names = [op["name"] for op in ops]
    muts = [op["name"] for op in ops if op["kind"] == "mut"]
    assert all(muts.count(m) == 1 for m in lo.MUTATORS if m not in ("set_prev_state", "set_defects_sparse"))
    assert set(lo.deferred_paths()) <= set(names)
    assert all(s["n"] <= 8 for s in lo.deferred_paths().values())


# ---- the second vocabulary (remelting, sub-stepped updates, the local loop, the timers) ------------------------------------------
# The scripts of the first vocabulary, operation for operation what they were before the second was added beside them:
# sha256(repr(make_script(L, name)))[:16] computed on the commit before it.
PINNED = {
    (16, 'pairs:a_rng0_full_cet_first'): 'e9d0bfb5fb8f3344', (16, 'pairs:a_rng0_incr_laser_inside'): '24ae86a0409dbfc3',
    (16, 'pairs:a_rng1_full_laser_none'): '58abd7569deaf324', (16, 'pairs:a_rng1_incr_cet_first20'): '503f67d0e3f4fa0b',
    (16, 'pairs:a_rng1_full_cet_last'): 'b43b2ff09674e734', (16, 'pairs:a_rng2_full_nothermal'): 'cf3cfb52c379ee95',
    (16, 'pairs:a_rng2_incr_laser_first'): '1652537abde2d4f7', (16, 'pairs:loop_single_calls'): '26b4f0e212c1f706',
    (16, 'pairs:b_box8'): '9d48fa4854c8c7ba', (16, 'pairs:b_box8_null_laser'): '80f0143d848ff4cd',
    (16, 'pairs:b_boxL'): 'd405ee026d226d6a', (16, 'pairs:b_boxL_null'): '8e2fea9968e732cd',
    (16, 'walk'): '92f7114f1e930837', (16, 'modes'): 'db7c5b1e5caa1254', (16, 'frozen'): 'c94129773fcb3671',
    (24, 'pairs:a_rng0_full_cet_first'): 'e9d0bfb5fb8f3344', (24, 'pairs:a_rng0_incr_laser_inside'): '24ae86a0409dbfc3',
    (24, 'pairs:a_rng1_full_laser_none'): '58abd7569deaf324', (24, 'pairs:a_rng1_incr_cet_first20'): '503f67d0e3f4fa0b',
    (24, 'pairs:a_rng1_full_cet_last'): 'b43b2ff09674e734', (24, 'pairs:a_rng2_full_nothermal'): 'cf3cfb52c379ee95',
    (24, 'pairs:a_rng2_incr_laser_first'): '1652537abde2d4f7', (24, 'pairs:loop_single_calls'): '26b4f0e212c1f706',
    (24, 'pairs:b_box8'): '9d48fa4854c8c7ba', (24, 'pairs:b_box8_null_laser'): '80f0143d848ff4cd',
    (24, 'pairs:b_boxL'): 'd405ee026d226d6a', (24, 'pairs:b_boxL_null'): '8e2fea9968e732cd',
    (24, 'pairs:b_box12'): 'd5b8ee9a49b66afa', (24, 'pairs:b_box12_null'): 'a9fd3ef3521184a7',
    (24, 'walk'): '98b3092cec75e437', (24, 'modes'): 'e8ff11108477b5ab', (24, 'frozen'): 'c94129773fcb3671',
    (136, 'pairs_deferred'): '50243fc6d7925f13',
}
NEW_CLASSES = set(lo.MUTATORS2.values())


def test_first_vocabulary_scripts_are_unchanged():
    import hashlib
    assert {(L, n) for L in SIZES for n in lo.script_names(L)} | {(136, "pairs_deferred")} == set(PINNED)
    for (L, name), want in PINNED.items():
        assert hashlib.sha256(repr(lo.make_script(L, name)).encode()).hexdigest()[:16] == want, (L, name)


def _crosses_update(spec, step0=None, n=None):
    step0, n = spec["step0"] if step0 is None else step0, spec["n"] if n is None else n
    return bool(spec.get("thermal_mode")) and lo.updates_before(step0, n) > 0


def _play2(oracle_mod, L, name):
    """Script ``name`` of the second vocabulary on the oracle: per-operation records and the runner as the script left it."""
    import substep_ref
    script = lo.make_script(L, name)
    r = lo.Runner(oracle_mod, L)
    recs = []
    for op, tag in zip(script, lo.tags(script, f"L={L} {name}")):
        rec = dict(op=op, tag=tag)
        if op["kind"] == "step":
            spec = r.paths[op["name"]]
            before = lo.clone(oracle_mod, r.lat)
            n_sub, melting = r.substeps, r.remelt_on
            n_ref = len(r.refusals)
            ro = r.do(op, tag)
            rec.update(ro=ro, spec=spec, refused=len(r.refusals) > n_ref, last=dict(r.last), melting=melting, substeps=n_sub)
            if ro is None:
                assert rec["refused"], tag
                recs.append(rec)
                continue
            rec["kinds"] = lo.event_kinds(spec, ro)
            inp = r.last.get("inp") or lo.step_inputs(L, spec, op["seed"])
            step0, n = r.last.get("args", (spec.get("step0"), spec["n"]))
            composed = "inp" in r.last                  # the call ran on the composed loop (a switch on, a cut, a marker)

            def again(c, n_sub, scale):
                if not composed:
                    return lo.oracle_step(c, spec, inp, scale)
                st = substep_ref.Stepper(c, n_sub, r.last["threshold"])
                st.applied_g = r.last["marker"]
                return st.run_steps(step0, n, lo.DEFECT_FRACTION, inp["u_pick"] * scale, inp["u_def"], inp["u_np"], rng_mode=spec["rng_mode"],
                                    seed=lo.COUNTER_SEED, thermal_mode=spec["thermal_mode"], thermal_dt=lo.THERMAL_DT, q_planes=inp["q"])

            if spec["kind"] == "loop" or (spec["kind"] == "run" and spec["rng_mode"] != 2):
                for scale in (1 - 1e-9, 1 + 1e-9):
                    rp = again(lo.clone(oracle_mod, before), n_sub, scale)
                    assert lo.event_key(spec, rp) == lo.event_key(spec, ro), f"{tag}: a pick flips with u_pick * {scale!r}: pick another seed"
            if composed and n_sub > 1 and _crosses_update(spec, step0, n) and not (r.last["marker"] == step0 and lo.updates_before(step0, n) == 1):
                c = lo.clone(oracle_mod, before)
                again(c, 1, 1.0)
                rec["T_differs_from_n1"] = c.T.tobytes() != r.lat.T.tobytes()
        else:
            cls = lo.MUTATORS2.get(op["name"]) or lo.MUTATORS.get(op["name"]) or ("options" if op["name"].startswith("opt_") else "read_only")
            sig = "impurity" if op["name"] == "param_impurity_c" else cls
            sig_before = lo.mutator_signature(oracle_mod, r.lat, sig)
            n_ref = len(r.refusals)
            r.do(op, tag)
            rec.update(cls=cls, changed=lo.mutator_signature(oracle_mod, r.lat, sig) != sig_before, last=dict(r.last),
                       refused=len(r.refusals) > n_ref)
        recs.append(rec)
    return recs, r


@pytest.fixture(scope="module")
def played2(oracle_mod):
    return {(L, n): _play2(oracle_mod, L, n) for L in SIZES for n in lo.script_names2(L)}


def test_second_vocabulary_occurs(played2):
    for L in SIZES:
        paths = set(lo.paths2(L))
        recs, _ = played2[(L, "walk2")]
        seen = [r["op"]["name"] for r in recs]
        everything = set(lo.MUTATORS) | set(lo.MUTATORS2) | set(lo.READ_ONLY) | set(lo.READ_ONLY2) | paths
        for x in everything:
            assert seen.count(x) >= 2, (L, "walk2", x, seen.count(x))
        assert 200 <= len(seen) <= 340, len(seen)
        for p in paths:          # pairs2: every M directly ahead of a call of S, which a call of S precedes
            names = [r["op"]["name"] for r in played2[(L, f"pairs2:{p}")][0]]
            assert names[0] == p
            for m in lo.MUTATORS2:
                hits = [q for q, x in enumerate(names) if x == m and names[q + 1:q + 2] == [p] and p in names[:q]]
                assert hits, (L, p, m)
        assert {"local"} == {lo.paths2(L)[p]["kind"] for p in ("local_k4", "local_k2_inf")}
    x = lo.extra_paths()
    assert (x["local_k4"]["K"], x["local_k4"]["thermal_mode"], x["local_k4"]["step0"] % 20) == (4, 1, 0) and np.isfinite(x["local_k4"]["horizon"])
    assert (x["local_k2_inf"]["K"], x["local_k2_inf"]["thermal_mode"], x["local_k2_inf"]["horizon"]) == (2, 0, np.inf)


def test_toggles_and_stopped_script_shapes(played2):
    for L in SIZES:
        recs, _ = played2[(L, "toggles")]
        runs = [r for r in recs if r["op"]["kind"] == "step" and r["spec"]["kind"] == "run"]
        assert all(r["spec"]["step0"] in (19, 20, 39) and _crosses_update(r["spec"]) for r in runs)
        combos = [(r["substeps"], r["melting"]) for r in runs]
        assert combos[:5] == [(1, False), (5, False), (5, True), (1, True), (1, False)] and (3, False) in combos[5:], combos
        assert runs[-1]["spec"]["incremental"] and {"super", "local"} <= {r["spec"]["kind"] for r in recs if r["op"]["kind"] == "step"}
        recs, _ = played2[(L, "stopped")]
        steps = [r for r in recs if r["op"]["kind"] == "step"]
        between = [r["op"]["name"] for q, r in enumerate(recs) if r["op"]["kind"] != "step" and 0 < q and "cut" in recs[q - 1]["op"]]
        assert between == [x for x in lo.STOPPED_KEEP + lo.STOPPED_DROP if x]
        for first, second in zip(steps[0::2], steps[1::2]):
            assert (first["ro"]["done"], first["ro"]["status"]) == (20, 2), first["tag"]
            assert (second["ro"]["done"], second["ro"]["status"]) == (first["spec"]["n"] - 20, 0), second["tag"]
            # the marker of the update that step 20 of the stopped batch applied: kept or dropped as INVALIDATES[] says
            assert second["last"]["marker"] == (20 if second["op"]["keeps"] else -1), second["tag"]
            assert second["ro"]["q_used"] == 1          # its plane is consumed (again, where the update is skipped)
        assert sum(s["op"].get("keeps", False) for s in steps) == len(lo.STOPPED_KEEP) and len(steps) == 2 * len(lo.STOPPED_KEEP + lo.STOPPED_DROP)


def test_second_vocabulary_stepping_calls_run_to_their_end(played2):
    for (L, name), (recs, _) in played2.items():
        refused = 0
        for r in _steps(recs):
            if r["refused"]:
                refused += 1
            elif name != "stopped":
                assert (r["ro"]["done"], r["ro"]["status"]) == (r["spec"]["n"], 0), r["tag"]
        if name.startswith("pairs2:") and lo._is_mode_b(lo.paths2(L)[name[7:]]):
            assert refused == 3, (L, name, refused)          # behind set_remelt_on, set_substeps=3 and set_substeps=5
    for L in SIZES:                  # the walk meets every documented refusal it can meet on one slab
        frags = {f for _, f in played2[(L, "walk2")][1].refusals}
        assert frags & {lo.REFUSED_MELT_ON, lo.REFUSED_SUBSTEPS} and lo.REFUSED_LOOKAHEAD in frags, (L, frags)


def test_new_mutators_change_what_they_must_and_no_ops_do_not(played2):
    for (L, name), (recs, r) in played2.items():
        assert r.min_gap >= 1e-9, (L, name, r.min_gap)
        for rec in recs:
            if rec["op"]["kind"] == "step" or rec["refused"]:
                continue
            if rec["cls"] in lo.NOOP_CLASSES2 or rec["cls"] == "read_only":
                assert not rec["changed"], rec["tag"]
            else:
                assert rec["changed"], rec["tag"]
            if rec["op"]["name"] in ("remelt", "time_remelt"):
                assert 3 <= rec["last"]["melted"] <= rec["last"]["occupied"] // 4, (rec["tag"], rec["last"])
            if rec["op"]["name"] == "remelt_nothing":
                assert rec["last"]["melted"] == 0, rec["tag"]


def test_melting_and_substepped_calls_do_something(played2):
    for (L, name), (recs, r) in played2.items():
        melting = [rec for rec in _steps(recs) if not rec["refused"] and rec["melting"] and rec["spec"]["kind"] == "run" and
                   "marker" in rec["last"] and _crosses_update(rec["spec"], *rec["last"]["args"]) and
                   not (rec["last"]["marker"] == rec["last"]["args"][0])]
        assert 2 * sum(rec["last"]["melted"] >= 1 for rec in melting) >= len(melting), (L, name, [rec["last"]["melted"] for rec in melting])
        if melting:
            assert (r.ever_melted & (r.lat.state != 0)).any(), (L, name, "no melted voxel is occupied again at the end")
        sub = [rec for rec in _steps(recs) if "T_differs_from_n1" in rec]
        assert all(rec["T_differs_from_n1"] for rec in sub), (L, name, [rec["tag"] for rec in sub if not rec["T_differs_from_n1"]])
        if name in ("toggles", "walk2") or (name.startswith("pairs2:a_") and _crosses_update(lo.paths2(L)[name[7:]])):
            assert melting and sub, (L, name, len(melting), len(sub))
        local = [rec for rec in _steps(recs) if not rec["refused"] and rec["spec"]["kind"] == "local"]
        if local:
            assert max(rec["last"]["max_per_box"] for rec in local) >= 2, (L, name)
        assert name not in ("toggles", "walk2", "pairs2:local_k4", "pairs2:local_k2_inf") or local


def test_nucleation_and_diffusion_right_behind_every_new_class(played2):
    for L in SIZES:
        first = {}
        for (l, name), (recs, _) in played2.items():
            if l != L or not (name.startswith("pairs2:") or name == "walk2"):
                continue
            script = "pairs2" if name.startswith("pairs2:") else name
            pending = set()          # the classes of the mutators since the last stepping call that ran
            for rec in recs:
                if rec["op"]["kind"] == "step":
                    if not rec["refused"]:
                        for cls in pending:
                            first.setdefault((script, cls), np.zeros(4, np.int64))
                            first[(script, cls)] += rec["kinds"]
                        pending = set()
                elif not rec["refused"] and rec["cls"] in NEW_CLASSES:
                    pending.add(rec["cls"])
        for script in ("pairs2", "walk2"):
            for cls in NEW_CLASSES:
                k = first[(script, cls)]
                assert k[1] >= 1 and k[2] >= 1, (L, script, cls, k)


def test_deferred_pairs2_script_shape():
    """The L > 128 case: every new mutator, setting and option once ahead of a deferring call, no more stepping calls than
    pairs_deferred has, and sub-stepped updates (n = 5) with no option set."""
    ops = lo.make_script(136, "pairs2_deferred")
    names = [op["name"] for op in ops]
    for m in lo.MUTATORS2:
        assert [q for q, x in enumerate(names) if x == m and names[q + 1:q + 2] and names[q + 1] in lo.deferred_paths()], m
    n_steps = lambda s: sum(op["kind"] == "step" for op in s)
    assert n_steps(ops) <= n_steps(lo.make_script(136, "pairs_deferred"))
    q = names.index("set_substeps=5")
    assert names[q + 1] in lo.deferred_paths() and not any(n.startswith("opt_substep") for n in names[:q])
