"""NumPy comparator of the canonical summation tree and of the selection that descends it, written from DESIGN.md
section 3 alone (neither from oracle/cet_oracle.c nor from the kernels) -- TEST INFRASTRUCTURE ONLY.

Input: an event list in reference order (plane i; block dep | diff | empty; j; k; slot), as ``Engine.enumerate_events`` and
``oracle.Lattice.enumerate`` return it, and L.  Every sum is made of np.float64 pairwise additions:

* voxel-category sum: sequential over the voxel's slots;
* row sum (i, c, j): balanced binary tree over k padded with zeros to next_pow2(L);
* block sum (i, c): balanced binary tree over j, same padding;
* total: balanced binary tree over the 3L blocks b = 3 i + c padded to a power of two;

an event count is carried beside every sum.  ``select(r)`` descends the same trees: at a node go left iff the right half
holds no events, or the left half holds events and base + sum(left) >= r; otherwise base += sum(left).  Inside the voxel
the slots are scanned (cum += rate; cum >= r), falling back to the last slot.  Every value that was compared with r on the
way is returned with its level, so a test can put r exactly on, one ulp below and one ulp above each of them.
"""
import numpy as np

LEVELS = ("block", "row", "voxel", "slot")
CATEGORY_OF_TYPE = np.array([0, 1, 2, 2])        # dep | diff | empty (nucleation, then attachments)


def next_pow2(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def _pad(a, P, dtype):
    out = np.zeros(a.shape[:-1] + (P,), dtype)
    out[..., :a.shape[-1]] = a
    return out


def _levels(vals, cnts):
    """Balanced tree over the last axis (a power of two long): [leaves, pairs, ..., root] of sums and of counts."""
    s, c = [vals], [cnts]
    with np.errstate(all="ignore"):
        while s[-1].shape[-1] > 1:
            s.append(s[-1][..., 0::2] + s[-1][..., 1::2])
            c.append(c[-1][..., 0::2] + c[-1][..., 1::2])
    return s, c


def _tree(vals, cnts):
    P = next_pow2(vals.shape[-1])
    return _levels(_pad(np.asarray(vals, np.float64), P, np.float64), _pad(np.asarray(cnts, np.int64), P, np.int64))


def _descend(tree, base, r, tag, thr, leaf=None):
    """One tree of the descent.  leaf None: steered by r (the rule of DESIGN.md section 3); otherwise towards that leaf.
    A threshold base + sum(left) is recorded where the rule compares it with r: both halves hold events."""
    s, c = tree
    idx = 0
    with np.errstate(all="ignore"):
        for d in range(len(s) - 2, -1, -1):
            left, right = 2 * idx, 2 * idx + 1
            sl = s[d][left]
            t = base + sl
            compared = c[d][right] != 0 and c[d][left] > 0
            if compared:
                thr.append((tag, t))
            if leaf is None:
                go_left = c[d][right] == 0 or (c[d][left] > 0 and t >= r)
            else:
                go_left = (leaf >> d) == left
            if go_left:
                idx = left
            else:
                base = t
                idx = right
    return idx, base


class Picked:
    """What a descent found.  index: position in the event list (None from RowTree); (i, c, j[, k]); base: the cumulative
    sum in front of the chosen voxel (RowTree: row); p_cum: the running sum including the chosen event; thresholds: [(level,
    value)] of everything compared with r on the way, in order."""

    def __init__(self, index, i, c, j, k, base, p_cum, thresholds):
        self.index, self.i, self.c, self.j, self.k, self.base, self.p_cum, self.thresholds = index, i, c, j, k, base, p_cum, thresholds


class RowTree:
    """The levels above the rows, from (L, 3, L) row sums and counts: block sums, total, and the descent to (i, c, j)."""

    def __init__(self, rowsum, rowcnt, L):
        self.L = L = int(L)
        self.rowsum = np.ascontiguousarray(rowsum, np.float64).reshape(3 * L, L)
        self.rowcnt = np.ascontiguousarray(rowcnt, np.int64).reshape(3 * L, L)
        rs, rc = _tree(self.rowsum, self.rowcnt)                 # every block's tree over j at once
        self._row_levels = (rs, rc)
        self.blocksum, self.blockcnt = rs[-1][:, 0].copy(), rc[-1][:, 0].copy()
        self._block_tree = _tree(self.blocksum, self.blockcnt)
        self.total = np.float64(self._block_tree[0][-1][0])
        self.n_events = int(self._block_tree[1][-1][0])

    def _row_tree(self, b):
        rs, rc = self._row_levels
        return [x[b] for x in rs], [x[b] for x in rc]

    def _to_row(self, r, thr, target=None):
        b, base = _descend(self._block_tree, np.float64(0.0), r, "block", thr, None if target is None else target[0])
        j, base = _descend(self._row_tree(b), base, r, "row", thr, None if target is None else target[1])
        return int(b), int(j), base

    def select_row(self, r):
        """(i, c, j) the pick r descends to, with the thresholds met."""
        assert self.n_events > 0
        thr = []
        b, j, base = self._to_row(np.float64(r), thr)
        return Picked(None, b // 3, b % 3, j, None, base, None, thr)

    def path_to_row(self, i, c, j):
        """The descent that ends at row (i, c, j) whatever r: its thresholds."""
        thr = []
        b, jj, base = self._to_row(None, thr, (3 * i + c, j))
        return Picked(None, i, c, jj, None, base, None, thr)


class SelectRef(RowTree):
    """The whole tree, from an event list in reference order."""

    def __init__(self, ev_type, ev_pos, ev_rate, L):
        L = int(L)
        typ = np.asarray(ev_type, np.int64)
        pos = np.asarray(ev_pos, np.int64).reshape(-1, 3)
        self.rate = np.ascontiguousarray(ev_rate, np.float64)
        n = len(typ)
        cat = CATEGORY_OF_TYPE[typ] if n else np.zeros(0, np.int64)
        row = (pos[:, 0] * 3 + cat) * L + pos[:, 1]
        key = row * L + pos[:, 2]
        assert np.all(np.diff(key) >= 0), "event list is not in reference order"
        # voxel-category sums: sequential over the voxel's slots
        self.vkey, self.vfirst, self.vcnt = np.unique(key, return_index=True, return_counts=True)
        self.vsum = np.zeros(len(self.vkey), np.float64)
        with np.errstate(all="ignore"):
            for s in range(int(self.vcnt.max()) if n else 0):
                m = self.vcnt > s
                self.vsum[m] = self.vsum[m] + self.rate[self.vfirst[m] + s]
        # row sums: balanced tree over k, rows that hold events only (every other row is zero / zero)
        P = next_pow2(L)
        rowsum, rowcnt = np.zeros(3 * L * L, np.float64), np.zeros(3 * L * L, np.int64)
        vrow, vk = self.vkey // L, self.vkey % L
        urow, ufirst = np.unique(vrow, return_index=True)
        uend = np.append(ufirst[1:], len(vrow))
        for a in range(0, len(urow), 4096):
            rows = urow[a:a + 4096]
            lo, hi = ufirst[a], uend[min(a + 4096, len(urow)) - 1]
            leaves, counts = np.zeros((len(rows), P), np.float64), np.zeros((len(rows), P), np.int64)
            at = np.searchsorted(rows, vrow[lo:hi])
            leaves[at, vk[lo:hi]] = self.vsum[lo:hi]
            counts[at, vk[lo:hi]] = self.vcnt[lo:hi]
            s, c = _levels(leaves, counts)
            rowsum[rows], rowcnt[rows] = s[-1][:, 0], c[-1][:, 0]
        super().__init__(rowsum.reshape(L, 3, L), rowcnt.reshape(L, 3, L), L)
        assert self.n_events == n

    def _voxel_tree(self, b, j):
        L = self.L
        row = b * L + j
        lo, hi = np.searchsorted(self.vkey, [row * L, (row + 1) * L])
        leaves, counts = np.zeros(L, np.float64), np.zeros(L, np.int64)
        k = self.vkey[lo:hi] - row * L
        leaves[k], counts[k] = self.vsum[lo:hi], self.vcnt[lo:hi]
        return _tree(leaves, counts), lo, k

    def _walk(self, r, target=None):
        thr = []
        tb = tj = tk = None
        if target is not None:
            v = int(np.searchsorted(self.vfirst, target, side="right")) - 1
            key = int(self.vkey[v])
            tb, tj, tk = key // (self.L * self.L), (key // self.L) % self.L, key % self.L
        b, j, base = self._to_row(r, thr, None if target is None else (tb, tj))
        tree, lo, ks = self._voxel_tree(b, j)
        k, base = _descend(tree, base, r, "voxel", thr, tk)
        v = lo + int(np.searchsorted(ks, k))
        assert self.vkey[v] == (b * self.L + j) * self.L + k
        first, cnt = int(self.vfirst[v]), int(self.vcnt[v])
        # slot scan: cum += rate; cum >= r; fallback to the last slot
        cum, pick, p_cum = base, first + cnt - 1, None
        with np.errstate(all="ignore"):
            for m in range(first, first + cnt):
                cum = cum + self.rate[m]
                thr.append(("slot", cum))
                p_cum = cum
                if (target is None and cum >= r) or (target is not None and m == target):
                    pick = m
                    break
        return Picked(pick, b // 3, b % 3, j, int(k), base, p_cum, thr)

    def select(self, r):
        """The event the pick r selects."""
        assert self.n_events > 0
        return self._walk(np.float64(r))

    def path_to(self, index):
        """The descent that ends at event ``index`` whatever r: its thresholds, base and p_cum."""
        return self._walk(None, int(index))

    def margin(self, r):
        """cetkmc_run_result.min_margin of a one-step call with the pick r: the distance of r from the nearer end of the
        chosen event's interval (p_cum - rate, p_cum], over the total -- in the kernel's operation order."""
        r = np.float64(r)
        p = self.select(r)
        with np.errstate(all="ignore"):
            lo = r - (p.p_cum - self.rate[p.index])
            hi = p.p_cum - r
            return (abs(lo) if abs(lo) < abs(hi) else abs(hi)) / self.total


def boundary_picks(t):
    """The three picks around a threshold t: one ulp below, on it, one ulp above."""
    t = np.float64(t)
    return [np.nextafter(t, -np.inf), t, np.nextafter(t, np.inf)]


def global_picks(total):
    """The picks at the ends of the whole range: 0, the total, one ulp above it, twice the total."""
    total = np.float64(total)
    return [np.float64(0.0), total, np.nextafter(total, np.inf), 2.0 * total]


def thresholds_of(ref, indices):
    """{level: [values]}: every distinct threshold met on the descents to the events ``indices``, in first-seen order."""
    seen = {}
    for m in indices:
        for level, t in ref.path_to(m).thresholds:
            seen.setdefault((level, float(t)), None)
    out = {level: [] for level in LEVELS}
    for level, t in seen:
        out[level].append(np.float64(t))
    return out


def event_sample(n_events, limit, seed):
    """Every event where there are at most ``limit``, otherwise ``limit`` seeded-random ones (ascending)."""
    if n_events <= limit:
        return np.arange(n_events)
    return np.sort(np.random.RandomState(seed).choice(n_events, limit, replace=False))


def picks_around(thresholds, total):
    """The distinct picks of a boundary test, ascending: one ulp below, on and one ulp above every threshold, then 0, the
    total, one ulp above it and twice the total."""
    vals = [r for t in thresholds for r in boundary_picks(t)] + global_picks(total)
    return np.unique(np.array(vals, np.float64))
