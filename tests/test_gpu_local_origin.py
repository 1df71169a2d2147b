"""The origin map behind the local event loop: the map the device folds from the loop's log (D * max_events records per
super-step ordinal) equals tests/origin_ref.py folded over the COMPARATOR's log, and a map changes nothing in the stepping."""
import numpy as np
import pytest

import local_ref as LR
import origin_ref as OR

pytestmark = pytest.mark.gpu
NAME = "L16_four_kinds"


def _engine():
    import cetkmc
    fields, L, tweak = LR.make_input_fields(NAME)
    params = cetkmc.default_params(LR.IMPURITY_C)
    for k, v in tweak.items():
        setattr(params, k, v)
    e = cetkmc.Engine(L, impurity_c=LR.IMPURITY_C, params=params)
    e.upload(*fields)
    return e


@pytest.mark.parametrize("want_events", [False, True])
def test_map_equals_the_fold_of_the_comparators_log(oracle_mod, want_events):
    L, _, _, hor, K, _, tm, df = LR.INPUTS[NAME]
    D = (L // 8) ** 3
    e = _engine()
    try:
        e.origin_begin()
        words, census, seq, step = np.zeros((L,) * 3, np.uint64), np.zeros((L, 5), np.int64), 0, LR.STEP0
        for n, (ro, state, *_rest) in zip(LR.BATCHES, LR.reference_run(oracle_mod, NAME)):
            rg = e.run_supersteps_local(step, n, df, LR.SEED, K, hor, thermal_mode=tm, want_events=want_events)
            assert rg["done"] == ro["done"] == n and ro["events"].shape == (n, D, K)
            seq = OR.absorb(words, census, ro["events"], seq, D * K, L)
            assert np.array_equal(e.origin_words(), words) and np.array_equal(e.origin_census(), census)
            assert e.origin_seq() == seq
            step += n
        assert seq == sum(LR.BATCHES) and census.sum() > seq
        _, code = OR.decode(words)
        assert set(np.unique(code)) >= {0, 3, 4, 5}              # attachments and hops (both ends) are on the map
    finally:
        e.close()


def test_a_map_perturbs_nothing():
    L, _, _, hor, K, _, tm, df = LR.INPUTS[NAME]
    out = []
    for with_map in (False, True):
        e = _engine()
        try:
            if with_map:
                e.origin_begin()
            res, step = [], LR.STEP0
            for n in LR.BATCHES:
                res.append(e.run_supersteps_local(step, n, df, LR.SEED, K, hor, thermal_mode=tm, want_events=True))
                step += n
            out.append((res, e.download(defects=True), e.rate_sweep(), e.nucleation_count(), e.counters()["supersteps"]))
        finally:
            e.close()
    (ra, fa, sa, na, ca), (rb, fb, sb, nb, cb) = out
    for a, b in zip(ra, rb):
        for k in ("events", "totals", "n_exec", "n_capped", "horizon", "dt_event"):
            assert a[k].tobytes() == b[k].tobytes(), k
    for k in fa:
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert (sa, na, ca) == (sb, nb, cb) and ca == sum(LR.BATCHES)
