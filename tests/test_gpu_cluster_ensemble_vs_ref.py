"""Ensemble.analyze against the independent comparator tests/cluster_ref.py and NumPy, replica by replica -- not through
Engine, whose single-lattice launches share the kernels: labels, first voxels, sizes and bounding boxes (the replicas' tables
are concatenated on the device), species counts and the species-3 gather (indices ascending, T bit-equal).  Lattices are
uploaded, not stepped.  L = 30 (27000 = 26 x 1024 + 376 voxels: the numbering kernel's last chunk is partial) with six
different replicas, one of them empty, one full, one of singletons; L = 64, where the 256-block launches stride; L = 17.

tests/test_cluster_ref_host.py checks these inputs without a GPU."""
import numpy as np
import pytest

import cluster_ref as CR

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("name", sorted(CR.ENSEMBLES))
def test_analyze_vs_ref(name):
    import cetkmc
    L, thresholds = CR.ENSEMBLES[name]
    reps = CR.ensemble_lattices(name)
    ens = cetkmc.Ensemble(L, [cetkmc.default_params() for _ in reps])
    for r, (state, theta, phi, T) in enumerate(reps):
        ens.replica(r).upload(state, theta, phi, T, np.zeros_like(state))
    for threshold in thresholds:
        an = ens.analyze(threshold, species=3, labels=True)
        assert len(an) == len(reps)
        for r, (state, theta, phi, T) in enumerate(reps):
            ref = CR.cluster_ref(state, theta, phi, threshold)
            CR.check_ensemble(name, r, state, ref)
            bad = CR.same(an[r]["clusters"], ref)
            assert bad == [], (r, threshold, bad, len(an[r]["clusters"]["size"]), len(ref["size"]))
            assert an[r]["counts"].tolist() == np.bincount(state.ravel(), minlength=6).tolist(), r
            idx, Tv = an[r]["gather"]
            want = np.flatnonzero(state.ravel() == 3)
            assert idx.dtype == np.int64 and np.array_equal(idx, want), r
            assert np.array_equal(_bits(Tv), _bits(T.ravel()[want])), r
        if name == "L30_R6":
            sizes = [len(a["clusters"]["size"]) for a in an]
            assert sizes[2] == 0 and min(sizes[:2] + sizes[3:]) > 0           # a zero-length entry inside the concatenated table
            assert len(an[3]["gather"][0]) == int((reps[3][0] != 0).sum())    # a replica entirely of the gathered species
