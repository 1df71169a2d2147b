"""The clustering comparator (tests/cluster_ref.py) and the host drop-in utils.get_clusters against the reference's own
clusterings (tests/golden/clusters_general.npz: continuous orientations, where grains form through chains of neighbours;
tests/golden/metrics.npz: palettes) and against each other at the threshold edges and on non-finite orientations; the
near-threshold guard; and, for every input of the GPU tests (test_gpu_cluster_vs_ref.py, test_gpu_cluster_ensemble_vs_ref.py)
at the exact shapes and seeds they use, the conditions without which a case could pass for a trivial reason."""
import numpy as np
import pytest

import cluster_ref as CR
from helpers import load

GENERAL_L = (8, 10, 12)
GENERAL_THRESHOLDS = (0.1, 0.5, 1.2, 4.0)


def _host(state, theta, phi, threshold):
    import utils
    with np.errstate(invalid="ignore"):
        clusters, visited = utils.get_clusters(np.asarray(state, np.int64), theta, phi, theta_threshold=threshold)
    return CR.from_host(clusters, visited)


def _check_fixture(z, key, in_key, threshold):
    state, theta, phi = z[in_key + "_state"].astype(np.int64), z[in_key + "_theta"], z[in_key + "_phi"]
    want_labels, want_size = z[key + "_visited"], z[key + "_cluster_sizes"].astype(np.int64)
    want_first = z[key + "_cluster_first"].reshape(-1, 3)
    ref = CR.cluster_ref(state, theta, phi, threshold)
    assert ref["ambiguous"] == 0
    host = _host(state, theta, phi, threshold)
    for name, got in (("cluster_ref", ref), ("utils.get_clusters", host)):
        assert np.array_equal(got["labels"], want_labels), (name, key)
        assert np.array_equal(got["size"], want_size), (name, key)
        assert np.array_equal(got["first"], want_first), (name, key)
    assert CR.same(host, ref) == []            # the bounding boxes too
    return ref


@pytest.mark.parametrize("L", GENERAL_L)
@pytest.mark.parametrize("threshold", GENERAL_THRESHOLDS)
def test_reference_fixture_continuous(L, threshold):
    ref = _check_fixture(load("clusters_general"), f"c_L{L}_t{threshold}", f"c_L{L}", threshold)
    if threshold in (0.5, 1.2):
        assert CR.chained_pairs(ref) > 0        # what the palette fixtures never have
    if threshold == 4.0:
        assert ref["join"].all() and len(ref["join"]) > 0


@pytest.mark.parametrize("name", ["m_L6", "m_L9", "m_L12", "m_empty"])
def test_reference_fixture_palette(name):
    _check_fixture(load("metrics"), name, name, 0.5)


@pytest.mark.parametrize("L,fill,seed", [(5, 1.0, 1), (9, 0.8, 2), (11, 0.6, 3)])
@pytest.mark.parametrize("threshold", [-1.0, 0.0, 0.1, 0.5, 1.2, float(np.pi), 4.0])
def test_ref_equals_host_continuous(L, fill, seed, threshold):
    state, theta, phi = CR.continuous(L, fill, seed)
    ref = CR.cluster_ref(state, theta, phi, threshold)
    assert ref["ambiguous"] == 0
    assert CR.same(_host(state, theta, phi, threshold), ref) == []
    n_occ = int((state != 0).sum())
    assert int(ref["size"].sum()) == n_occ
    if threshold <= 0.0:
        assert len(ref["size"]) == n_occ
    if threshold > np.pi:
        assert ref["join"].all()


def test_ref_equals_host_nonfinite():
    rng = np.random.default_rng(5)
    state, theta, phi = CR.continuous(9, 0.9, 4)
    at = rng.choice(state.size, 60, replace=False)
    theta.ravel()[at[:20]] = np.nan
    phi.ravel()[at[20:40]] = np.inf
    theta.ravel()[at[40:]] = -np.inf
    assert CR.nonfinite_next_to_finite(state, theta, phi) > 0
    for threshold in (0.0, 0.5, 1.2, float(np.pi), 4.0):
        ref = CR.cluster_ref(state, theta, phi, threshold)
        assert ref["ambiguous"] == 0
        assert CR.same(_host(state, theta, phi, threshold), ref) == []
        bad = (state != 0) & ~(np.isfinite(theta) & np.isfinite(phi))
        assert bad.any() and (ref["size"][ref["labels"][bad] - 1] == 1).all()          # a non-finite voxel joins nothing


@pytest.mark.parametrize("threshold", [0.5, 0.1, 1.2])
def test_guard_fires_on_planted_pair(threshold):
    """one pair of voxels, equal phi, theta apart by threshold + d: ambiguous for |d| = 1e-14, not for |d| = 1e-10."""
    for off in CR.FORWARD:
        for d, want in ((1e-14, 1), (-1e-14, 1), (1e-10, 0), (-1e-10, 0)):
            state = np.zeros((4, 4, 4), np.int64)
            theta, phi = np.zeros((4, 4, 4)), np.full((4, 4, 4), 0.9)
            a = (1, 1, 1)
            b = tuple(x + o for x, o in zip(a, off))
            state[a] = state[b] = 1
            theta[a], theta[b] = 0.8, 0.8 + threshold + d
            ref = CR.cluster_ref(state, theta, phi, threshold)
            assert len(ref["a"]) == 1
            assert ref["ambiguous"] == want, (off, d)
            if not want:
                assert len(ref["size"]) == (1 if d < 0 else 2), (off, d)
    # NaN is never ambiguous, and neither is anything at the thresholds that do not compare cosines
    theta[a] = np.nan
    assert CR.cluster_ref(state, theta, phi, threshold)["ambiguous"] == 0
    theta[a] = theta[b]
    for thr in (-1.0, 0.0, 4.0):
        assert CR.cluster_ref(state, theta, phi, thr)["ambiguous"] == 0


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("L,fill,threshold,seed", CR.GENERAL)
def test_inputs_general(L, fill, threshold, seed):
    state, theta, phi = CR.continuous(L, fill, seed)
    ref = CR.cluster_ref(state, theta, phi, threshold)
    CR.check_general(ref, L, threshold)
    assert int(ref["size"].sum()) == int((state != 0).sum())
    if L == 130:
        assert state.size > 8192 * 256          # past the launch grid's cap: the grid-stride loops iterate


def test_inputs_edge_lattice():
    state, theta, phi = CR.edge_lattice()
    assert CR.nonfinite_next_to_finite(state, theta, phi) > 0
    n_occ = int((state != 0).sum())
    for threshold in CR.EDGE_THRESHOLDS:
        ref = CR.cluster_ref(state, theta, phi, threshold)
        assert ref["ambiguous"] == 0, threshold
        assert CR.same(_host(state, theta, phi, threshold), ref) == []
        if threshold <= 0.0:
            assert len(ref["size"]) == n_occ
        else:
            assert 1 < len(ref["size"]) < n_occ
    # equal palette vectors: dot products at (or an ulp from) 1.0, which joins at every positive threshold
    ref = CR.cluster_ref(state, theta, phi, 0.1)
    assert ref["join"].sum() > 100


@pytest.mark.parametrize("threshold", [0.5, 0.1])
def test_inputs_planted_pairs(threshold):
    state, theta, phi, pairs = CR.planted_pairs(threshold)
    assert len(pairs) == 28 and int((state != 0).sum()) == 56
    ref = CR.cluster_ref(state, theta, phi, threshold)
    assert ref["ambiguous"] == 0
    assert len(ref["a"]) == 28                                  # every pair alone: no other stencil pair in the lattice
    for a, b, sign in pairs:
        assert (ref["labels"][a] == ref["labels"][b]) == (sign < 0), (a, b, sign)
    assert len(ref["size"]) == 14 + 2 * 14
    assert CR.same(_host(state, theta, phi, threshold), ref) == []


@pytest.mark.parametrize("L", [33, 64])
def test_inputs_serpentine(L):
    one = CR.serpentine(L)
    ref = CR.cluster_ref(*CR.constant(one), CR.CONST_THRESHOLD)
    CR.check_serpentine(ref, one, 1)
    assert tuple(ref["first"][0]) == (0, 0, 0)
    deg = CR.join_degree(ref)
    assert deg[0] == 1 and np.count_nonzero(deg == 1) == 2      # a path: two ends, the first voxel is one of them
    two = one | CR.serpentine(L, 1)
    ref2 = CR.cluster_ref(*CR.constant(two), CR.CONST_THRESHOLD)
    CR.check_serpentine(ref2, two, 2)
    assert np.array_equal(ref2["labels"] == 1, one)


def test_inputs_connectivity():
    L = 64
    ref = CR.cluster_ref(*CR.constant(np.ones((L, L, L), bool)), CR.CONST_THRESHOLD)
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    assert ref["ambiguous"] == 0 and len(ref["size"]) == 2
    assert np.array_equal(ref["labels"], 1 + (i + j + k) % 2)
    occ = CR.mod4(L)
    ref = CR.cluster_ref(*CR.constant(occ), CR.CONST_THRESHOLD)
    assert ref["ambiguous"] == 0 and len(ref["size"]) == int(occ.sum()) == 16 ** 3
    for L in (1, 2, 3):
        state, theta, phi = CR.constant(np.ones((L, L, L), bool))
        ref = CR.cluster_ref(state, theta, phi, CR.CONST_THRESHOLD)
        assert CR.same(_host(state, theta, phi, CR.CONST_THRESHOLD), ref) == []
        assert len(ref["size"]) == (1 if L == 1 else 2)          # the two parities of i + j + k


@pytest.mark.parametrize("name", sorted(CR.ENSEMBLES))
def test_inputs_ensembles(name):
    L, thresholds = CR.ENSEMBLES[name]
    reps = CR.ensemble_lattices(name)
    for threshold in thresholds:
        for r, (state, theta, phi, T) in enumerate(reps):
            CR.check_ensemble(name, r, state, CR.cluster_ref(state, theta, phi, threshold))
    if name == "L30_R6":
        assert (reps[1][0] != 0).all()
    assert any(np.isnan(T[st == 3]).any() and np.isinf(T[st == 3]).any() for st, _, _, T in reps)


def test_inputs_textured_and_sites():
    CR.check_textured(CR.cluster_ref(*CR.textured(), 0.5))
    lat = CR.site_lattices()
    mixed, one = lat["mixed"][0], lat["one"][0]
    assert mixed.size > 1024 * 256              # past the 1024-block launches of the site queries
    assert [int((mixed == s).sum()) > 0 for s in range(5)] == [True, True, True, True, False]
    assert (one == 2).all()
    for state, _, _, T, _ in lat.values():
        for s in np.unique(state):
            t = T[state == s]
            assert np.isnan(t).any() and np.isposinf(t).any() and np.isneginf(t).any()
