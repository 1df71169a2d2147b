"""The origin maps of a replica ensemble: cetkmc_run_ensemble absorbs every replica's executed steps in one launch.  Every
replica is checked against the comparator (origin_ref.py) fed with its own ORACLE log; one replica terminates in its first
step (frozen at once: its map stays empty) and one starts from an empty lattice.  A replica's bytes equal those of the same
lattice stepped on a single handle; the batched profile after an analysis and after an import, the replica handles' own
calls, the batched census and the handle rules."""
import numpy as np
import pytest

import layer_ref as LR
import origin_ref as OR
import test_gpu_ensemble_vs_oracle as EO
from helpers import FOUR_KIND_PARAMS, random_lattice, step_uniforms

pytestmark = pytest.mark.gpu

FIELDS = tuple(f for f in OR.REC_FIELDS if f != "pad")
CALLS = ((0, 25), (25, 15))
DEFECT_FRACTION = 0.05


def _diff(got, want):
    return [f for f in FIELDS if not np.array_equal(got[f], want[f])]


@pytest.mark.parametrize("R,L", [(5, 12), (3, 33)])
def test_ensemble_vs_oracle(oracle_mod, R, L):
    import cetkmc
    fz, empty = 0, 1
    lattices = []
    for r in range(R):
        lat = random_lattice(L, 50 + r)
        if r == fz:
            # defect voxels only: no event is possible, the replica terminates in its first step
            lat = (np.full((L,) * 3, 4, np.int64), np.zeros((L,) * 3), np.zeros((L,) * 3), np.full((L,) * 3, 3000.0),
                   np.zeros((L,) * 3, np.int64))
        if r == empty:
            lat = (np.zeros((L,) * 3, np.int64), np.zeros((L,) * 3), np.zeros((L,) * 3), lat[3], np.zeros((L,) * 3, np.int64))
        lattices.append(lat)
    imp = [0.05 * (r % 4) for r in range(R)]
    run = EO._Run(oracle_mod, L, lattices, imp, defect_fraction=DEFECT_FRACTION, tweak=FOUR_KIND_PARAMS, rng_mode=0, thermal_mode=1)
    ens = run.ens
    one = None
    try:
        with pytest.raises(RuntimeError, match="needs the maps"):
            ens.origin_census()
        assert (ens.origin_seq() == -1).all()
        with pytest.raises(RuntimeError, match="single-lattice handle"):
            ens.replica(R - 1).origin_begin()
        ens.origin_begin()
        with pytest.raises(RuntimeError, match="single-lattice handle"):
            ens.replica(R - 1).origin_end()
        words = [np.zeros((L,) * 3, np.uint64) for _ in range(R)]
        census = np.zeros((R, L, 5), np.int64)
        seq = [0] * R
        for step0, n in CALLS:
            res, ros = run.call(step0, n)
            for r in range(R):
                if ros[r] is not None:
                    seq[r] = OR.absorb(words[r], census[r], ros[r]["events"], seq[r], 1, L)
            assert ros[fz] is None or (ros[fz]["status"], ros[fz]["done"]) == (1, 0), "the frozen replica"
        assert seq[fz] == 0 and not words[fz].any() and seq[empty] == 40 and seq[R - 1] == 40
        assert np.array_equal(ens.origin_seq(), seq)
        assert np.array_equal(ens.origin_census(), census)
        for r in range(R):
            assert np.array_equal(ens.replica(r).origin_words(), words[r]), r
            assert np.array_equal(ens.replica(r).origin_census(), census[r]), r
        both = ens.origin_read()
        assert both["ordinal"].shape == (R, L, L, L) and np.array_equal(both["code"][R - 1], OR.decode(words[R - 1])[1])
        states = [np.array(run.lats[r].state, np.int64) for r in range(R)]

        # the batched profile behind the batched analysis, and behind an import
        an = ens.analyze(0.5, labels=True)
        got = ens.origin_profile(grains=True, recluster=False)
        again = ens.origin_profile(grains=True, recluster=False)
        plain = ens.origin_profile()
        assert plain["grains"] is None
        for r in range(R):
            lab = an[r]["clusters"]["labels"]
            lay, gr = OR.profile(words[r], states[r], lab, len(an[r]["clusters"]["size"]))
            assert _diff({f: got["layers"][f][r] for f in FIELDS}, lay) == [] and _diff(got["grains"][r], gr) == [], r
            assert _diff({f: plain["layers"][f][r] for f in FIELDS}, lay) == [], r
            assert all(got["grains"][r][f].tobytes() == again["grains"][r][f].tobytes() for f in FIELDS)
            assert np.array_equal(gr["n_occ"], an[r]["clusters"]["size"])
            if r > 0:              # the replica handle's own profile (replica 0's handle is the ensemble's: refused)
                pr = ens.replica(r).origin_profile()
                assert _diff(pr["layers"], lay) == [], r
        with pytest.raises(RuntimeError, match="ensemble handle"):
            ens.replica(0).origin_profile()
        labs = []
        for r in range(R):
            raw, _ = LR.labelling(LR.KINDS[r % len(LR.KINDS)], L, r)
            labs.append(LR.from_raw(raw)[0].astype(np.int32))
        ens.import_clusters(np.stack(labs))
        got = ens.origin_profile(grains=True, recluster=False)
        for r in range(R):
            lay, gr = OR.profile(words[r], states[r], labs[r], int(labs[r].max()))
            assert _diff({f: got["layers"][f][r] for f in FIELDS}, lay) == [] and _diff(got["grains"][r], gr) == [], r

        # the same lattice on a single handle: the same calls, the same streams -- the same bytes
        r = R - 1
        one = cetkmc.Engine(L, params=run.params[r])
        one.upload(*lattices[r])
        one.origin_begin()
        for c, (step0, n) in enumerate(CALLS):
            u = step_uniforms(1000 * c + r, n, max(n * (L * L + 2), 1))
            out = one.run_steps(step0, n, DEFECT_FRACTION, *u, rng_mode=0, thermal_mode=1)
            assert (out["done"], out["status"]) == (n, 0)
        assert one.origin_words().tobytes() == words[r].tobytes() and one.origin_census().tobytes() == census[r].tobytes()
        one.import_clusters(labs[r])
        p1 = one.origin_profile(grains=True, recluster=False)
        assert all(p1["grains"][f].tobytes() == got["grains"][r][f].tobytes() for f in FIELDS)
        assert all(p1["layers"][f].tobytes() == got["layers"][f][r].tobytes() for f in FIELDS)

        ens.origin_begin()                                     # a second begin resets every replica's map and clock
        assert not ens.origin_census().any() and not ens.origin_seq().any() and not ens.replica(R - 1).origin_words().any()
        ens.origin_end()
        with pytest.raises(RuntimeError, match="needs a map"):
            ens.replica(1).origin_words()
    finally:
        if one is not None:
            one.close()
        run.close()
