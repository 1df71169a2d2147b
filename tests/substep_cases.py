"""Inputs of the sub-stepping GPU tests (tests/test_gpu_substep_*.py), shared with tests/test_substep_ref_host.py, which
asserts on the comparator alone (tests/substep_ref.py) that each of them holds what it is meant to exercise: a NaN in front of
sub-step 1, voxels on either clip value after some sub-step, a latent-heat release, a non-zero source.

The temporally blocked kernel (csrc/thermal_sub.hpp) writes tiles of (32 - 2 S) rows x (128 - 2 S) columns, S <= 4 sub-steps
per launch: 26 x 122 at S = 3, the default at L > 128.  Up to L = 128 the default is one launch per sub-step (measured faster
there), so the tests of small lattices ask for the blocked kernel by option (BLOCKED below); the plane group is set by option
substep_planes (PLANES) where a test wants more than one group in a small lattice.
"""
import functools

import numpy as np

from oracle import oracle
import remelt_cases as rc
import substep_ref

S_DEFAULT, S_MAX, PLAIN_L = 3, 4, 128
TJ, TK, PLANES = 32 - 2 * S_DEFAULT, 128 - 2 * S_DEFAULT, 8
BLOCKED = {"substep_block": S_DEFAULT}


def default_block(L):
    """sub-steps per launch a one-slab handle of edge L takes without option substep_block (1: the plain path)"""
    return S_DEFAULT if L > PLAIN_L else 1


# L = 1, 2, 3, 5; T - 1, T, T + 1 for the plane group (7, 8, 9 with substep_planes = 8), the tile rows (25, 26, 27) and the tile
# columns (121, 122, 123); 2 TJ + 1 = 53; 129 (the general kernel behind a tile multiple) and 256 (sub-step 1 = the fused tiles)
SMALL_SIZES = (1, 2, 3, 5, PLANES - 1, PLANES, PLANES + 1, TJ - 1, TJ, TJ + 1, 2 * TJ + 1)
LARGE_SIZES = (TK - 1, TK, TK + 1, 129)
# (n - 1) % S takes every remainder: n in {1, 2, S, S + 1, S + 2, 2 S + 1, 17}
SUBSTEPS = (1, 2, S_DEFAULT, S_DEFAULT + 1, S_DEFAULT + 2, 2 * S_DEFAULT + 1, 17)
CLIP_LO, CLIP_HI = float(oracle.T_SUB), oracle.T_MELT * 1.1


def noisy_gradient(L, seed=0, lo=3000.0, hi=3600.0, noise=50.0):
    """a linear gradient over the planes with +- noise K per voxel: the rough field of the stability table"""
    rs = np.random.RandomState(seed)
    return lo + (hi - lo) * np.arange(L)[:, None, None] / max(L - 1, 1) + rs.uniform(-noise, noise, (L, L, L))


@functools.lru_cache(maxsize=4)
def direct_fields(L):
    """(state, theta, phi, T, defects), prev_state, q: a lattice of rc.block_lattice's kind with a rough field that spans the
    whole clip range (so that every update leaves voxels on both clip values), one occupied voxel in five freshly filled
    (prev_state 0 there) and a source plane with its peak on the lattice corner (j, k) = (0, 0)"""
    state, theta, phi, _, defects = rc.block_lattice(L, 40 + L, sparse=0.3)
    T = noisy_gradient(L, seed=L, lo=CLIP_LO + 10.0, hi=CLIP_HI - 10.0)
    if L == 1:
        T[:] = 3333.0
    rs = np.random.RandomState(7 + L)
    prev = np.where(rs.random_sample(state.shape) < 0.2, 0, state)
    if not ((prev == 0) & (state != 0)).any():
        state[0, 0, 0], prev[0, 0, 0] = 1, 0
    q = oracle.laser_source_plane(L, (L - 1, 0), 60.0)
    return (state, theta, phi, T, defects), prev, q


def nonfinite_sites(L):
    """a face, an edge, a corner and a seam of the S = 3 tile (rows 25 | 26, columns 121 | 122 where the lattice has them)"""
    m = L - 1
    sites = [(L // 2, 0, L // 2), (0, 0, L // 2), (m, m, m)]
    sites += [(L // 2, min(TJ - 1, m), min(TK - 1, m)), (L // 3, min(TJ, m), min(TK, m))]
    return sorted(set(sites))


def with_nonfinite(T, L):
    """T with NaN and +inf alternating over nonfinite_sites(L)"""
    T = T.copy()
    for q, v in enumerate(nonfinite_sites(L)):
        T[v] = np.nan if q % 2 == 0 else np.inf
    return T


def direct_reference(L, n, mode, use_latent=True, scrub=True, nonfinite=False, updates=1, threads=1):
    """the comparator's field after `updates` updates of direct_fields(L) in n sub-steps, and what they exercised"""
    fields, prev, q = direct_fields(L)
    T0 = with_nonfinite(fields[3], L) if nonfinite else fields[3]
    lat = oracle.Lattice(fields[0], fields[1], fields[2], T0, fields[4], impurity_c=0.1)
    lat.prev_state = np.ascontiguousarray(prev, np.int8)
    stats = substep_ref.new_stats()
    oracle.set_threads(threads)
    try:
        for _ in range(updates):
            substep_ref.update(lat, n, 1e-6, mode, q, use_latent=use_latent, scrub=scrub, stats=stats)
    finally:
        oracle.set_threads(1)
    return lat.T, stats


# ---- stepping (tests/test_gpu_substep_stepping.py): remelt_cases' lattices and calls, a threshold only where remelting is on ----
def _case(name, base, n_sub, remelt=False, **over):
    c = dict(rc.STEPPING[base] if base in rc.STEPPING else rc.ENSEMBLE[base])
    c.update(over)
    c.update(name=name, n_sub=n_sub, remelt=remelt)
    return c


STEPPING = {c["name"]: c for c in (
    _case("L24_laser_latent_rng0_full_n3", "L24_laser_latent_rng0_full", 3),
    _case("L24_laser_latent_rng0_full_n17", "L24_laser_latent_rng0_full", 17),
    _case("L24_laser_nolatent_rng1_incr_n17", "L24_laser_nolatent_rng1_incr", 17),
    _case("L24_cet_rng1_incr_n3", "L24_laser_nolatent_rng1_incr", 3, thermal_mode=1),
    _case("L40_cet_rng2_full_n17_remelt", "L40_cet_lowered_rng2_full", 17, remelt=True),
    _case("L40_cet_rng2_full_n3", "L40_cet_lowered_rng2_full", 3),
    _case("L136_laser_latent_deferred_n3", "L136_laser_latent_deferred", 3),
    _case("L256_fused_tiles_n3", "L256_fused_tiles", 3),
)}
ENSEMBLE = {c["name"]: c for c in (
    _case("ens_L30_n3", "ens_L30", 3),
    _case("ens_L33_n17", "ens_L33", 17),
)}


def run_case(case, variant=0, seed_off=0, power=60.0, lat0=None):
    """the comparator's run of a case, in the shape of rc.run_case (results and fields after every call)"""
    oracle.set_threads(case["threads"])
    try:
        lat0 = rc.lattice_of(case, variant) if lat0 is None else lat0
        lat = oracle.Lattice(*lat0, impurity_c=0.1)
        st = substep_ref.Stepper(lat, case["n_sub"], case["threshold"] if case["remelt"] else None)
        calls, results, fields, nucs = rc.calls_of(case, power), [], [], []
        for (s0, n, up, ud, unp, q) in calls:
            results.append(st.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"] + seed_off,
                                        thermal_mode=case["thermal_mode"], q_planes=q, use_latent=case["use_latent"]))
            fields.append(tuple(a.copy() for a in (lat.state, lat.theta, lat.phi, lat.T, lat.prev_state)))
            nucs.append(lat.nuc_count)
            if results[-1]["status"]:
                break
        return dict(lat0=lat0, calls=calls, results=results, fields=fields, nucs=nucs, stepper=st)
    finally:
        oracle.set_threads(1)


@functools.lru_cache(maxsize=None)
def stepped(name, variant=0, seed_off=0, power=60.0):
    return run_case({**STEPPING, **ENSEMBLE}[name], variant, seed_off, power)
