"""Comparator of the origin map (include/cetkmc.h, cetkmc_origin_*): pure NumPy, integers only.

    absorb(words, census, events, seq, group, L)   folds event records into the words and the census, in place
    profile(words, state, labels, n)               the per-plane and per-grain records

It shares no code with the library or its binding: the record layouts are restated here."""
import numpy as np

DEP, NUC, ATT, HOP, LEFT = 1, 2, 3, 4, 5
CODE_OF_TYPE = np.array([DEP, 0, NUC, ATT], np.int64)      # event type 0 dep, 1 diff, 2 nuc, 3 att
INT64_MAX = np.iinfo(np.int64).max
SEQ_LIMIT = 1 << 36

EVENT = np.dtype([("type", "<i4"), ("pos", "<i4", 3), ("target", "<i4", 3), ("atom", "<i4"), ("rate", "<f8"),
                  ("dep_rank", "<i8"), ("theta", "<f8"), ("phi", "<f8")], align=True)
REC_FIELDS = ("n_occ", "n_by", "n_unrec", "n_left", "ord_sum", "ord_min", "ord_max", "birth", "pad")
REC = np.dtype([("n_occ", "<i8"), ("n_by", "<i8", 4), ("n_unrec", "<i8"), ("n_left", "<i8"), ("ord_sum", "<i8"),
                ("ord_min", "<i8"), ("ord_max", "<i8"), ("birth", "<i8"), ("pad", "<i8")])
assert EVENT.itemsize == 64 and REC.itemsize == 96


def enc(ordinal, code):
    """The word of a record: ((ordinal + 1) << 3) | code."""
    return ((np.asarray(ordinal, np.uint64) + np.uint64(1)) << np.uint64(3)) | np.asarray(code, np.uint64)


def decode(words):
    """(ordinal, -1 for none; code) of words."""
    w = np.asarray(words, np.uint64)
    return (w >> np.uint64(3)).astype(np.int64) - 1, (w & np.uint64(7)).astype(np.int64)


def make_events(rows):
    """EVENT records from (type, pos, target) rows; target None = (-1, -1, -1)."""
    ev = np.zeros(len(rows), EVENT)
    for q, (t, pos, tgt) in enumerate(rows):
        ev[q]["type"] = t
        ev[q]["pos"] = pos
        ev[q]["target"] = (-1, -1, -1) if tgt is None else tgt
        ev[q]["dep_rank"] = -1
    return ev


def absorb(words, census, events, seq, group, L):
    """Folds ``events`` (any shape, row-major order) into ``words`` (L, L, L) uint64 and ``census`` (L, 5) int64, in place:
    records [g * group, (g + 1) * group) carry the ordinal seq + g.  Returns the new seq."""
    ev = np.asarray(events).reshape(-1)
    n = len(ev)
    assert group >= 1 and n % group == 0
    assert words.dtype == np.uint64 and words.shape == (L, L, L) and census.dtype == np.int64 and census.shape == (L, 5)
    steps = n // group
    assert seq + steps < SEQ_LIMIT
    if n == 0:
        return seq
    w = words.reshape(-1)
    t = ev["type"].astype(np.int64)
    pos, tgt = ev["pos"].astype(np.int64), ev["target"].astype(np.int64)
    ordinal = seq + np.arange(n, dtype=np.int64) // group
    ok = (t >= 0) & (t <= 3)
    diff = ok & (t == 1) & (tgt[:, 0] >= 0)
    fill = ok & (t != 1)
    assert np.all((pos[fill | diff] >= 0) & (pos[fill | diff] < L)) and np.all((tgt[diff] >= 0) & (tgt[diff] < L))
    lin_p = (pos[:, 0] * L + pos[:, 1]) * L + pos[:, 2]
    lin_t = (tgt[:, 0] * L + tgt[:, 1]) * L + tgt[:, 2]
    np.maximum.at(w, lin_p[fill], enc(ordinal[fill], CODE_OF_TYPE[t[fill]]))
    np.maximum.at(w, lin_p[diff], enc(ordinal[diff], LEFT))
    np.maximum.at(w, lin_t[diff], enc(ordinal[diff], HOP))
    np.add.at(census, (pos[fill | diff, 0], t[fill | diff]), 1)
    np.add.at(census, (tgt[diff, 0], np.full(int(diff.sum()), 4)), 1)
    return seq + steps


def _records(n_rec, key, w, lin, occupied, left):
    """n_rec records over voxels with record index ``key``, words w, linear indices lin; ``occupied`` voxels are classified by
    their word, ``left`` voxels count in n_left."""
    r = np.zeros((n_rec, 12), np.int64)
    r[:, 8] = r[:, 10] = INT64_MAX
    r[:, 9] = -1
    o, code = decode(w)
    fill = occupied & (code >= DEP) & (code <= HOP)
    np.add.at(r[:, 0], key[occupied], 1)
    for c in (DEP, NUC, ATT, HOP):
        np.add.at(r[:, c], key[fill & (code == c)], 1)
    np.add.at(r[:, 5], key[occupied & ~fill], 1)
    np.add.at(r[:, 6], key[left], 1)
    np.add.at(r[:, 7], key[fill], o[fill])
    np.minimum.at(r[:, 8], key[fill], o[fill])
    np.maximum.at(r[:, 9], key[fill], o[fill])
    np.minimum.at(r[:, 10], key[fill], (o[fill] << 27) | (code[fill] << 24) | lin[fill])
    return np.ascontiguousarray(r).view(REC).reshape(n_rec)


def profile(words, state, labels=None, n=0):
    """(layers REC[L], grains REC[n] or None) of the map ``words`` over the lattice ``state``, grain records by ``labels``
    (ids 1..n; anything else counts in no grain)."""
    L = words.shape[0]
    assert L ** 3 <= 1 << 24
    w = np.asarray(words, np.uint64).reshape(-1)
    s = np.asarray(state).reshape(-1)
    lin = np.arange(L ** 3, dtype=np.int64)
    plane = lin // (L * L)
    code = (w & np.uint64(7)).astype(np.int64)
    layers = _records(L, plane, w, lin, s != 0, (s == 0) & (code == LEFT))
    if labels is None:
        return layers, None
    g = np.asarray(labels).reshape(-1).astype(np.int64)
    m = (g >= 1) & (g <= n)
    grains = _records(int(n), g[m] - 1, w[m], lin[m], np.ones(int(m.sum()), bool), np.zeros(int(m.sum()), bool))
    return layers, grains
