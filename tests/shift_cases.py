"""Inputs shared by the cetkmc_shift tests (tests/test_shift_ref_host.py asserts, on the comparator alone, what they claim)."""
import numpy as np

import shift_ref

CALL_SIZES = (1, 2, 3, 7, 8, 9, 33, 64, 65, 129, 136, 264)
MIXED = ((3, -5, 9), (-2, 0, 1), (0, 8, -8))
NAN_PAYLOAD_BITS = 0x7FF8DEADBEEF1234          # a quiet NaN with a payload
NEG_NAN_BITS = -0x000700000000ABCD             # sign bit set, payload (int64 view of 0xFFF8FFFFFFFF5433)


def call_shifts(L):
    """every d of test_gpu_shift_call at edge L: each axis alone by +-1, +-7, +-8, +-9, +-(L - 1), +-L and L + 3, and the
    mixed shifts; without duplicates and without d = 0 (L = 1: L - 1 = 0)"""
    out = []
    for a in range(3):
        for m in (1, 7, 8, 9, L - 1, L):
            for sgn in (1, -1):
                d = [0, 0, 0]
                d[a] = sgn * m
                out.append(tuple(d))
        d = [0, 0, 0]
        d[a] = L + 3
        out.append(tuple(d))
    out += list(MIXED)
    seen, uniq = set(), []
    for d in out:
        if d != (0, 0, 0) and d not in seen:
            seen.add(d)
            uniq.append(d)
    return uniq


def special_fields(L, seed):
    """dict of the five fields: a random lattice of all five states with a defect mask, and in T, theta and phi a NaN with
    a payload, a negative NaN, +inf, -inf and -0.0 scattered over the lattice (corners and faces among the places)"""
    rs = np.random.RandomState(seed)
    n = L ** 3
    state = rs.choice([0, 1, 2, 3, 4], size=(L, L, L), p=[0.5, 0.25, 0.1, 0.1, 0.05]).astype(np.int64)
    defects = ((state == 3) & (rs.random_sample((L, L, L)) < 0.5)).astype(np.int64)
    out = dict(state=state, defects=defects)
    specials = np.array([NAN_PAYLOAD_BITS, NEG_NAN_BITS], np.int64).view(np.float64).tolist() + [np.inf, -np.inf, -0.0]
    for name, lo, hi in (("theta", 0.0, np.pi), ("phi", 0.0, 2 * np.pi), ("T", 2600.0, 3900.0)):
        a = rs.uniform(lo, hi, n)
        bits = a.view(np.int64)
        for q, sp in enumerate(specials):
            # places: the first and last voxel, and a stride through the lattice
            idx = np.unique(np.concatenate([[q % n, (n - 1 - q) % n], np.arange(q * 3 + 1, n, 61 + 7 * q)]))
            bits[idx] = np.array([sp], np.float64).view(np.int64)[0]
        out[name] = a.reshape(L, L, L)
    return out


def physical_fields(L, seed):
    """dict of the five fields of helpers.random_lattice: finite everywhere, all four event families present"""
    from helpers import random_lattice
    st, th, ph, T, df = random_lattice(L, seed)
    return dict(state=st, theta=th, phi=ph, T=T, defects=df)


def seam_zone(L, d):
    """exposed voxels and every voxel within two voxels (any direction) of the seam"""
    ex = ~shift_ref.inside_mask(L, d)

    def grown(m):
        p = np.pad(m, 2)
        out = np.zeros_like(m)
        for a in range(5):
            for b in range(5):
                for c in range(5):
                    out |= p[a:a + L, b:b + L, c:c + L]
        return out
    return ex | (grown(ex) & grown(~ex))


def events_in_zone(L, d, events):
    zone = seam_zone(L, d)
    ev = np.asarray(events).reshape(-1)
    n = 0
    for x in ev:
        if x["type"] < 0:
            continue
        n += int(zone[tuple(x["pos"])])
        if x["type"] == 1 and x["target"][0] >= 0:
            n += int(zone[tuple(x["target"])])
    return n
