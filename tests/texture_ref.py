"""NumPy comparator of the texture profile (cetkmc_texture_profile) and the inputs its tests use.

``texture_ref`` restates the definition with whole-array comparisons of shifted volumes -- no tiles, no rims, no histograms
in shared memory: nothing of the device kernel's structure.  The unit vectors come from theta / phi as the reference's
compute_misorientation forms them (sin / cos products).

The counters are integers, but they bin floating-point values, and the device's sincos and NumPy's sin / cos differ by a few
ulp.  With |components| <= 1 that bounds the difference of a dot product d or a pole value c by about 3e-15.  A value that
close to an edge may fall on either side, so a test first asserts, on the comparator alone, that none of ITS values lies
within ``guard`` = 1e-12 of an edge (:func:`ambiguous`; more than 300 times the bound), and then compares with ==.  An input
that trips the assertion is replaced by another input; the guard stays.
"""
import numpy as np

import layer_ref as LR

FIELDS = ("gb_hist", "pole_hist", "bad")
GUARD = 1e-12


def vectors(theta, phi):
    """(..., 3) unit vectors (sin t cos p, sin t sin p, cos t); NaN where an angle is not finite."""
    theta, phi = np.asarray(theta, np.float64), np.asarray(phi, np.float64)
    with np.errstate(invalid="ignore"):
        st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
    return np.stack([st * cp, st * sp, ct], axis=-1)


def edges_cos(n_bins, span_deg):
    """the n_bins - 1 interior edges of n_bins equal steps over 0..span_deg as cosines (strictly decreasing)."""
    return np.cos(np.deg2rad(np.arange(1, n_bins, dtype=np.float64) * (float(span_deg) / n_bins)))


def bin_of(x, edges):
    """the binning rule: the number of edges with x <= e[q] (edges strictly decreasing)."""
    x = np.asarray(x, np.float64)
    return (x[..., None] <= np.asarray(edges, np.float64).reshape(-1)).sum(axis=-1)


def ambiguous(values, edges, guard=GUARD):
    """how many (value, edge) pairs are closer than ``guard``: such a value could be binned either way by a few ulp."""
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    return int(sum(np.count_nonzero(np.abs(v - e) <= guard) for e in np.asarray(edges, np.float64).reshape(-1)))


def face_values(labels, theta, phi):
    """per axis a: (plane index i of v, d) of every grain-grain face (v, predecessor u of v along a: both labels non-zero
    and different), d = o(u)[0]*o(v)[0] + o(u)[1]*o(v)[1] + o(u)[2]*o(v)[2] summed left to right."""
    g = np.asarray(labels, np.int64)
    L = g.shape[0]
    o = vectors(theta, phi)
    plane = np.broadcast_to(np.arange(L).reshape(L, 1, 1), g.shape)
    out = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, L - 1), slice(1, L)
        lo, hi = tuple(lo), tuple(hi)
        face = (g[hi] != 0) & (g[lo] != 0) & (g[hi] != g[lo])
        u, v = o[lo], o[hi]
        d = (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]
        out.append((plane[hi][face], d[face]))
    return out


def pole_values(labels, theta, phi, axis):
    """(plane index, c) of every occupied voxel, c = fabs(axis[0]*o[0] + axis[1]*o[1] + axis[2]*o[2])."""
    g = np.asarray(labels, np.int64)
    L = g.shape[0]
    o = vectors(theta, phi)
    ax = [float(x) for x in axis]
    c = np.abs((ax[0] * o[..., 0] + ax[1] * o[..., 1]) + ax[2] * o[..., 2])
    occ = g != 0
    return np.broadcast_to(np.arange(L).reshape(L, 1, 1), g.shape)[occ], c[occ]


def _hist(plane, x, edges, L, n_bins):
    """(hist (L, n_bins), bad (L,)) of the values x of the planes ``plane``"""
    ok = np.isfinite(x)
    h = np.zeros((L, n_bins), np.int64)
    np.add.at(h, (plane[ok], bin_of(x[ok], edges)), 1)
    return h, np.bincount(plane[~ok], minlength=L).astype(np.int64)


def texture_ref(labels, theta, phi, gb_edges, pole_edges, axis=(1.0, 0.0, 0.0), values=None):
    """The per-plane histograms of one lattice: dict of int64 arrays gb_hist (L, 3, n_bins), pole_hist (L, n_bins), bad
    (L, 4).  ``values``: (face_values, pole_values) computed before (they do not depend on the edges)."""
    L = np.asarray(labels).shape[0]
    n_bins = len(np.asarray(gb_edges).reshape(-1)) + 1
    assert len(np.asarray(pole_edges).reshape(-1)) == n_bins - 1
    faces, pole = values if values is not None else (face_values(labels, theta, phi), pole_values(labels, theta, phi, axis))
    out = {"gb_hist": np.zeros((L, 3, n_bins), np.int64), "pole_hist": None, "bad": np.zeros((L, 4), np.int64)}
    for a in range(3):
        out["gb_hist"][:, a, :], out["bad"][:, a] = _hist(faces[a][0], faces[a][1], gb_edges, L, n_bins)
    out["pole_hist"], out["bad"][:, 3] = _hist(pole[0], pole[1], pole_edges, L, n_bins)
    return out


def n_ambiguous(values, gb_edges, pole_edges):
    """near-edge values of a lattice's (face_values, pole_values) against the two edge arrays"""
    faces, pole = values
    return sum(ambiguous(d, gb_edges) for _, d in faces) + ambiguous(pole[1], pole_edges)


def same(got, want):
    """list of (field, plane) where two profiles differ (empty: equal in every counter)."""
    bad = []
    for k in FIELDS:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == np.int64, (k, a.shape, b.shape, a.dtype)
        bad += [(k, int(i)) for i in np.unique(np.argwhere(a != b)[:, 0])]
    return bad


# ---- inputs --------------------------------------------------------------------------------------------------------------
def random_angles(L, s=0):
    """theta ~ U(0, pi), phi ~ U(0, 2 pi) per voxel from default_rng(1000 + L + s)."""
    rng = np.random.default_rng(1000 + L + s)
    return rng.uniform(0.0, np.pi, (L, L, L)), rng.uniform(0.0, 2.0 * np.pi, (L, L, L))


def checker(L, w=(3, 3, 5), off=(1, 2, 3)):
    """Offset checkerboard: cells of w[a] voxels along axis a, the cell faces across an axis shifted by off[a] and by the next
    coordinate (a sheared board), so that along every block edge of the kernel (8 rows, 32 columns, 16 planes) some voxel
    pairs lie in one cell and others in two; a cell's raw id is (c0 + 2 c1 + 3 c2) % 4, id 0 empty.  Returns the raw volume
    (layer_ref.from_raw makes it importable)."""
    i, j, k = np.meshgrid(np.arange(L), np.arange(L), np.arange(L), indexing="ij")
    c0, c1, c2 = (i + j + off[0]) // w[0], (j + k + off[1]) // w[1], (k + i + off[2]) // w[2]
    return ((c0 + 2 * c1 + 3 * c2) % 4).astype(np.int64)


KINDS = ("scattered", "stripes0", "stripes1", "stripes2", "checker")
# the kernel's block edges (csrc/texture.hpp: TEX_TJ rows, TEX_TK columns, TEX_NI planes): (axis, last index before the edge)
EDGES = ((1, 7), (2, 31), (0, 15))


def labelling(kind, L):
    """an importable labelling (int32, ids 1..n by first occurrence, 0 = empty) of one of KINDS."""
    raw = checker(L) if kind == "checker" else LR.labelling(kind, L, LR.case_seed(kind, L))[0]
    return LR.from_raw(raw)[0].astype(np.int32)


def check_not_vacuous(kind, L, labels):
    """same-label and other-label predecessor pairs lie across every block edge of the kernel that the lattice reaches (the
    random partition and the checkerboard have both sorts at every edge; slabs have one sort per axis)."""
    for axis, at in EDGES:
        if L > at + 1:
            same_pair, other_pair = LR.straddles(labels, axis, at)
            if kind in ("scattered", "checker"):
                assert same_pair and other_pair, (kind, L, axis)
            else:
                assert same_pair or other_pair, (kind, L, axis)
