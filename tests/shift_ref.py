"""NumPy comparator of cetkmc_shift (include/cetkmc.h): voxel v of the old lattice moves to v + d.

Everything is index arithmetic and copies: no value is computed, so every comparison against it is ``==`` (doubles by
their int64 views).  Written from the rule alone, per axis with ``np.take`` -- it shares nothing with the kernels.
"""
import numpy as np

FIELDS = ("state", "defects", "theta", "phi", "T")


def source_index(L, d):
    """per axis a: (clamped source index s_a = v_a - d_a for every v_a, inside mask)"""
    out = []
    for a in range(3):
        s = np.arange(L, dtype=np.int64) - int(d[a])
        out.append((np.clip(s, 0, L - 1), (s >= 0) & (s < L)))
    return out


def inside_mask(L, d):
    """(L, L, L) bool: the source v - d of voxel v lies in the lattice"""
    (_, mi), (_, mj), (_, mk) = source_index(L, d)
    return mi[:, None, None] & mj[None, :, None] & mk[None, None, :]


def gather(a, d):
    """a[clamp(v - d)] for every v: the old array continued outward (trailing axes beyond the third ride along)"""
    L = a.shape[0]
    (si, _), (sj, _), (sk, _) = source_index(L, d)
    return np.take(np.take(np.take(a, si, axis=0), sj, axis=1), sk, axis=2)


def shift_array(a, d, fill):
    """moved array: exposed entries are ``fill``; the bits of everything kept are untouched"""
    a = np.ascontiguousarray(a)
    ins = inside_mask(a.shape[0], d)
    out = gather(a, d).copy()
    out[~ins] = fill
    return out


def _bits_fill(x):
    return np.array([x], dtype=np.float64).view(np.int64)[0]


def shift_f64(a, d, fill):
    """as shift_array for doubles, through int64 views: NaN payloads and -0.0 survive, also in the fill"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    return shift_array(a.view(np.int64), d, _bits_fill(fill)).view(np.float64)


def shift_fields(f, d, fill_state=0, fill_T=300.0, T_mode="value", fill_theta=0.0, fill_phi=0.0):
    """f: dict of the five (L, L, L) fields.  Returns (new fields, info) with info = dict(kept, exposed, dropped[6])."""
    L = f["state"].shape[0]
    d = [int(x) for x in d]
    ins = inside_mask(L, d)
    out = dict(state=shift_array(f["state"], d, fill_state), defects=shift_array(f["defects"], d, 0),
               theta=shift_f64(f["theta"], d, fill_theta), phi=shift_f64(f["phi"], d, fill_phi))
    if T_mode == "value":
        out["T"] = shift_f64(f["T"], d, fill_T)
    elif T_mode == "edge":
        out["T"] = gather(np.ascontiguousarray(f["T"], dtype=np.float64).view(np.int64), d).view(np.float64).copy()
    else:
        raise ValueError(T_mode)
    # an old voxel v leaves when v + d is outside: the inside mask of the opposite move
    leaves = ~inside_mask(L, [-x for x in d])
    st = np.asarray(f["state"])[leaves]
    dropped = [int((st == x).sum()) for x in range(5)]
    dropped.append(int(st.size) - sum(dropped))
    exposed = int((~ins).sum())
    return out, dict(kept=L ** 3 - exposed, exposed=exposed, dropped=dropped)


def shift_solid(m, d):
    """m: dict(stamp (L,L,L) int64, T_s, g (L,L,L,3), cool) as Engine.solid_read returns them"""
    return dict(stamp=shift_array(np.asarray(m["stamp"], dtype=np.int64), d, -1), T_s=shift_f64(m["T_s"], d, 0.0),
                g=shift_f64(m["g"], d, 0.0), cool=shift_f64(m["cool"], d, 0.0))


def shift_origin_words(words, d):
    return shift_array(np.asarray(words, dtype=np.uint64), d, 0)


def shift_census(census, d):
    """census (L, 5): the rows move along axis 0 by d[0], zero fill"""
    c = np.asarray(census, dtype=np.int64)
    L = c.shape[0]
    out = np.zeros_like(c)
    for i in range(L):
        s = i - int(d[0])
        if 0 <= s < L:
            out[i] = c[s]
    return out
