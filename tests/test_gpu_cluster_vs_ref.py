"""Engine.clusters (csrc/cluster.hpp: lock-free union-find) against the independent comparator tests/cluster_ref.py --
labels, sizes, first voxels and bounding boxes, all compared with == -- on inputs the older tests do not have: continuous
orientations (grains that hold together only through chains of neighbours), lattices past the launch grid's cap (L = 130),
thresholds at and beyond both ends, pairs 1e-10 rad from the threshold, non-finite orientations, and shapes that are pure
connectivity (two percolating parity classes, singletons, one long thin path).  Then the product path
(metrics.compute_metrics_device) and the sparse site queries at L = 70.

tests/test_cluster_ref_host.py checks, without a GPU, that every input used here has no pair within the comparator's guard
of the threshold and meets the conditions that keep its case from passing for a trivial reason; the cheap ones are asserted
here again from the comparator's output."""
import functools

import numpy as np
import pytest

import cluster_ref as CR

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _continuous(L, fill, seed):
    return CR.continuous(L, fill, seed)


@functools.lru_cache(maxsize=None)
def _general_ref(L, fill, threshold, seed):
    return CR.cluster_ref(*_continuous(L, fill, seed), threshold)


def _engine(state, theta, phi):
    import cetkmc
    e = cetkmc.Engine(state.shape[0])
    e.upload(state, theta, phi, np.full(state.shape, 3000.0), np.zeros_like(state))
    return e


def _compare(e, ref, threshold):
    assert ref["ambiguous"] == 0
    got = e.clusters(threshold, labels=True)
    assert got["size"].dtype == np.int64 and got["first"].dtype == np.int32 and got["bbox"].dtype == np.int32
    bad = CR.same(got, ref)
    assert bad == [], (bad, len(got["size"]), len(ref["size"]), np.argwhere(got["labels"] != ref["labels"])[:4].tolist())
    return got


@pytest.mark.parametrize("L,fill,threshold,seed", CR.GENERAL)
def test_general(L, fill, threshold, seed):
    ref = _general_ref(L, fill, threshold, seed)
    CR.check_general(ref, L, threshold)
    _compare(_engine(*_continuous(L, fill, seed)), ref, threshold)


@pytest.mark.parametrize("threshold", CR.EDGE_THRESHOLDS)
def test_threshold_edges_and_nonfinite(threshold):
    state, theta, phi = CR.edge_lattice()
    assert CR.nonfinite_next_to_finite(state, theta, phi) > 0
    ref = CR.cluster_ref(state, theta, phi, threshold)
    _compare(_engine(state, theta, phi), ref, threshold)
    bad = (state != 0) & ~(np.isfinite(theta) & np.isfinite(phi))
    assert (ref["size"][ref["labels"][bad] - 1] == 1).all()


@pytest.mark.parametrize("threshold", [0.5, 0.1])
def test_planted_pairs_near_threshold(threshold):
    """Pairs 1e-9 and 1e-10 rad either side of the threshold: at 0.5 that is 4.8e-11 in the cosine -- outside the comparator's
    guard, far inside single precision."""
    state, theta, phi, pairs = CR.planted_pairs(threshold)
    ref = CR.cluster_ref(state, theta, phi, threshold)
    for a, b, sign in pairs:
        assert (ref["labels"][a] == ref["labels"][b]) == (sign < 0)
    _compare(_engine(state, theta, phi), ref, threshold)


def test_full_lattice_two_parities():
    L = 64
    lat = CR.constant(np.ones((L, L, L), bool))
    ref = CR.cluster_ref(*lat, CR.CONST_THRESHOLD)
    assert ref["size"].tolist() == [L ** 3 // 2] * 2
    _compare(_engine(*lat), ref, CR.CONST_THRESHOLD)


def test_singletons():
    lat = CR.constant(CR.mod4(64))
    ref = CR.cluster_ref(*lat, CR.CONST_THRESHOLD)
    assert len(ref["size"]) == int((lat[0] != 0).sum()) > 0
    _compare(_engine(*lat), ref, CR.CONST_THRESHOLD)


@pytest.mark.parametrize("L", [33, 64])
@pytest.mark.parametrize("n_paths", [1, 2])
def test_serpentine(L, n_paths):
    occ = CR.serpentine(L) if n_paths == 1 else CR.serpentine(L) | CR.serpentine(L, 1)
    lat = CR.constant(occ)
    ref = CR.cluster_ref(*lat, CR.CONST_THRESHOLD)
    CR.check_serpentine(ref, occ, n_paths)
    _compare(_engine(*lat), ref, CR.CONST_THRESHOLD)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_tiny(L):
    for occ in (np.ones((L, L, L), bool), np.zeros((L, L, L), bool)):
        lat = CR.constant(occ)
        _compare(_engine(*lat), CR.cluster_ref(*lat, CR.CONST_THRESHOLD), CR.CONST_THRESHOLD)


def test_empty_after_nonempty_and_repeat():
    """One engine: a clustering with many grains, the same call again (identical), an empty lattice (nothing of the earlier
    tables may show), and the first lattice once more."""
    L, fill, threshold, seed = CR.GENERAL[1]
    lat, ref = _continuous(L, fill, seed), _general_ref(L, fill, threshold, seed)
    e = _engine(*lat)
    first = _compare(e, ref, threshold)
    again = _compare(e, ref, threshold)
    for k in ("labels", "size", "first", "bbox"):
        assert np.array_equal(first[k], again[k]), k
    zero = np.zeros_like(lat[0])
    e.upload(zero, lat[1], lat[2], np.full(zero.shape, 3000.0), zero)
    got = e.clusters(threshold, labels=True)
    assert len(got["size"]) == 0 and got["first"].shape == (0, 3) and got["bbox"].shape == (0, 6)
    assert not got["labels"].any()
    e.upload(lat[0], lat[1], lat[2], np.full(zero.shape, 3000.0), zero)
    ref2 = CR.cluster_ref(*lat, 0.5)
    _compare(e, ref2, 0.5)
    _compare(e, ref, threshold)


def test_product_metrics_percolating():
    """metrics.compute_metrics_device (fixed threshold 0.5) on a lattice whose largest grain percolates, against the same
    dict computed from the comparator's clustering."""
    import metrics
    lat = CR.textured()
    ref = CR.cluster_ref(*lat, 0.5)
    CR.check_textured(ref)
    n_def = int((lat[0] == 3).sum())
    want = metrics.compute_metrics_from_clusters(ref, lat[0].size, defects_count=n_def)
    got = metrics.compute_metrics_device(_engine(*lat), lat[0].size, defects_count=n_def)
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["GrainCount"] == len(ref["size"]) > 1


# ---- sparse site queries at L = 70 (343000 voxels: past the 1024 x 256 threads of their launches) --------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _sites():
    return CR.site_lattices()


@pytest.mark.parametrize("n_slabs", [1, 3])
@pytest.mark.parametrize("name", ["mixed", "one"])
def test_species_counts_and_gather(n_slabs, name):
    import cetkmc
    state, theta, phi, T, dm = _sites()[name]
    e = cetkmc.Engine(CR.SITE_L, n_slabs=n_slabs)
    e.upload(state, theta, phi, T, dm)
    counts = e.species_counts()
    assert counts.tolist() == np.bincount(state.ravel(), minlength=6).tolist()
    for s in range(5):
        idx, Tv = e.gather_species(s)
        want = np.flatnonzero(state.ravel() == s)
        assert idx.dtype == np.int64 and np.array_equal(idx, want), s
        assert np.array_equal(_bits(Tv), _bits(T.ravel()[want])), s
    assert len(e.gather_species(4)[0]) == 0
    if name == "one":
        assert len(e.gather_species(2)[0]) == state.size


@pytest.mark.parametrize("n_slabs", [1, 3])
def test_set_defects_sparse(n_slabs):
    import cetkmc
    state, theta, phi, T, dm = _sites()["mixed"]
    e = cetkmc.Engine(CR.SITE_L, n_slabs=n_slabs)
    e.upload(state, theta, phi, T, dm)
    rng = np.random.default_rng(71)
    idx = rng.integers(0, state.size, 5000)
    idx = np.concatenate([idx, idx[:700], [0, state.size - 1, 0]])       # duplicates, both ends of the lattice
    rng.shuffle(idx)
    assert len(np.unique(idx)) < len(idx) and (np.diff(idx) < 0).any()
    mask = np.zeros(state.size, np.int64)
    mask[idx] = 1

    def flags():
        return e.download(state=False, theta=False, phi=False, T=False, defects=True)["defects"]

    e.set_defects_sparse(idx)
    assert np.array_equal(flags(), mask.reshape(state.shape))
    e.set_defects_sparse(np.zeros(0, np.int64))
    assert not flags().any()
    e.set_defects_sparse(idx[:10])
    assert int(flags().sum()) == len(np.unique(idx[:10]))


def test_clusters_refused_on_two_slabs():
    import cetkmc
    state, theta, phi = _continuous(*[CR.GENERAL[1][q] for q in (0, 1, 3)])
    e = cetkmc.Engine(state.shape[0], n_slabs=2)
    e.upload(state, theta, phi, np.full(state.shape, 3000.0), np.zeros_like(state))
    with pytest.raises(RuntimeError, match="one slab"):
        e.clusters(0.5)
    assert e.species_counts().tolist() == np.bincount(state.ravel(), minlength=6).tolist()
    assert np.array_equal(e.download()["state"], state)
