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
