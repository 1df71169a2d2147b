"""Inputs of the implicit-scheme GPU tests (tests/test_gpu_implicit_*.py), shared with tests/test_implicit_ref_host.py, which
asserts on the comparator alone (tests/implicit_ref.py) what each of them exercises.

Seams of csrc/thermal_imp.hpp, beside the sizes the scheme's definition asks for (1, 2, 3, 5, 31..33, 63..65, 127..129, 256):
  k_imp_rows   chunks of C = 64 columns (63 | 64 | 65: one chunk, exactly one, one and a column; 127..129: the second chunk) and
               blocks of 64 rows that run across planes (every L that 64 does not divide; L = 5: one partial block; L = 8: one
               full block; L = 31: fifteen blocks and one row)
  k_imp_lines  loads issued U = 8 elements ahead from element 1 on: L - 1 = 7, 8, 9 and 16 (L = 8, 9, 10, 17)
"""
import functools

import numpy as np

from oracle import oracle
import implicit_ref
import remelt_cases as rc
from substep_ref import new_stats

CHUNK, ROWS, AHEAD = 64, 64, 8
SIZES = (1, 2, 3, 5, 8, 9, 10, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SUBSTEPS = (1, 2, 3)
CLIP_LO, CLIP_HI = float(oracle.T_SUB), oracle.T_MELT * 1.1
POWER = 300.0                # of the direct calls' source (about 1050 K per update at the peak): the voxels under the beam
                             # land on T_clip_hi, and an L = 5 lattice still keeps voxels on T_clip_lo
DT = 1e-6


@functools.lru_cache(maxsize=4)
def direct_fields(L):
    """(state, theta, phi, T, defects), prev_state, q: a lattice of rc.block_lattice's kind; a rough field over the whole clip
    range whose lowest planes lie BELOW T_clip_lo (the scheme cannot leave the input's range, so only such an input reaches
    the lower clip value); one occupied voxel in five freshly filled; a source with its peak on the lattice corner (0, 0)"""
    state, theta, phi, _, defects = rc.block_lattice(L, 140 + L, sparse=0.3)
    rs = np.random.RandomState(900 + L)
    T = rs.uniform(CLIP_LO + 10.0, CLIP_HI - 10.0, (L, L, L))
    T[:max(L // 4, 1)] = rs.uniform(CLIP_LO - 900.0, CLIP_LO - 600.0, (max(L // 4, 1), L, L))
    prev = np.where(rs.random_sample(state.shape) < 0.2, 0, state)
    if not ((prev == 0) & (state != 0)).any():
        state[0, 0, 0], prev[0, 0, 0] = 1, 0
    q = oracle.laser_source_plane(L, (L - 1, 0), POWER)
    return (state, theta, phi, T, defects), prev, q


def nonfinite_sites(L):
    """a face, an edge, a corner and the seam of the 64-column chunk (k = 63 | 64 where the lattice has them)"""
    m = L - 1
    sites = [(L // 2, 0, L // 2), (0, 0, L // 2), (m, m, m), (0, m, 0)]
    sites += [(L // 2, L // 3, min(CHUNK - 1, m)), (L // 3, L // 2, min(CHUNK, m))]
    return sorted(set(sites))


def with_nonfinite(T, L, only_nan=False):
    """T with NaN, +inf and -inf in turn over nonfinite_sites(L); only_nan: one NaN, at the first site"""
    T = T.copy()
    sites = nonfinite_sites(L)
    if only_nan:
        T[sites[0]] = np.nan
        return T
    for n, v in enumerate(sites):
        T[v] = (np.nan, np.inf, -np.inf)[n % 3]
    return T


def direct_lattice(L, nonfinite=False, only_nan=False):
    fields, prev, q = direct_fields(L)
    T0 = with_nonfinite(fields[3], L, only_nan) if (nonfinite or only_nan) else fields[3]
    lat = oracle.Lattice(fields[0], fields[1], fields[2], T0, fields[4], impurity_c=0.1)
    lat.prev_state = np.ascontiguousarray(prev, np.int8)
    return lat, T0, prev, q


@functools.lru_cache(maxsize=None)
def direct_reference(L, n, mode, use_latent=True, scrub=True, nonfinite=False, only_nan=False, updates=1):
    """the comparator's field after `updates` updates of the direct input in n implicit steps, and what they exercised"""
    lat, _, _, q = direct_lattice(L, nonfinite, only_nan)
    stats = new_stats()
    for _ in range(updates):
        implicit_ref.update(lat, n, DT, mode, q, use_latent=use_latent, scrub=scrub, stats=stats)
    return lat.T, stats


# ---- stepping: remelt_cases' lattices and calls.  Every case begins on an update step (step0 a multiple of 20), so the update
# stands in front of every rate evaluation, and every lattice is uploaded with a NaN, a +inf, a block below T_clip_lo and a block
# above T_clip_hi in it (plant): the scheme cannot leave the input's range, so only such inputs land on the clip values.  The
# hot block lies in the interior, not under the beam: an EMPTY top-plane voxel between about 3900 K and 3925 K has a deposition
# rate near the largest double (rc.block_lattice), and a source strong enough to lift the top plane to T_clip_hi puts a ring of
# such voxels around the beam -- the totals reach 1e308 and overflow (at 300 W the L = 24 latent case stops with an infinite
# total in its third call), which is no input to compare sums on within 1e-11. ----
def _case(name, base, n_sub, remelt=False, **over):
    c = dict(rc.STEPPING[base] if base in rc.STEPPING else rc.ENSEMBLE[base])
    c.update(over)
    c.update(name=name, n_sub=n_sub, remelt=remelt)
    assert c["step0"] % 20 == 0, name
    return c


STEPPING = {c["name"]: c for c in (
    _case("L24_laser_latent_rng0_full_n1", "L24_laser_latent_rng0_full", 1),
    _case("L24_laser_latent_rng0_full_n3", "L24_laser_latent_rng0_full", 3),
    _case("L24_laser_nolatent_rng1_incr_n1", "L24_laser_nolatent_rng1_incr", 1),
    _case("L24_cet_rng1_incr_n3", "L24_laser_nolatent_rng1_incr", 3, thermal_mode=1),
    _case("L40_cet_rng2_full_n1_remelt", "L40_cet_lowered_rng2_full", 1, remelt=True),
    _case("L40_cet_rng2_full_n3", "L40_cet_lowered_rng2_full", 3),
    _case("L136_laser_latent_deferred_n1", "L136_laser_latent_deferred", 1, step0=0),
    _case("L256_fused_tiles_n1", "L256_fused_tiles", 1, step0=20),
)}
ENSEMBLE = {c["name"]: c for c in (
    _case("ens_L30_n1", "ens_L30", 1, step0=20),
    _case("ens_L33_n3", "ens_L33", 3, step0=20),
)}
POWERS = (60.0, 80.0)       # the two plane sets of the ensemble cases


def plant(lat0):
    """the lattice with planes 0..2 of one quadrant 700 K below T_clip_lo, three interior planes of the opposite quadrant 700 K
    above T_clip_hi, a NaN on a face and a +inf on an edge"""
    state, theta, phi, T, defects = lat0
    L = T.shape[0]
    h, a = L // 2, L // 3
    T = np.array(T, np.float64)
    T[:3, :h, :h] = CLIP_LO - 700.0
    T[a:a + 3, h:, h:] = CLIP_HI + 700.0
    T[h, 0, h], T[0, L - 1, 0] = np.nan, np.inf
    return state, theta, phi, T, defects


def lattice_of(case, variant=0):
    return plant(rc.lattice_of(case, variant))


def run_case(case, variant=0, seed_off=0, power=60.0, lat0=None):
    """the comparator's run of a case, in the shape of rc.run_case (results and fields after every call); a lattice of the
    caller's is planted like the case's own"""
    oracle.set_threads(case["threads"])
    try:
        lat0 = lattice_of(case, variant) if lat0 is None else plant(lat0)
        lat = oracle.Lattice(*lat0, impurity_c=0.1)
        st = implicit_ref.Stepper(lat, case["n_sub"], case["threshold"] if case["remelt"] else None)
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


def _full_cold(L):
    """no event anywhere (every voxel occupied): terminates in the call's first step"""
    rs = np.random.RandomState(77)
    state = rs.randint(1, 4, (L, L, L)).astype(np.int64)
    ang = rs.random_sample((L, L, L))
    return state, ang, 2 * ang, np.full((L, L, L), 3000.0), np.zeros_like(state)


def _empty(case):
    z = np.zeros((case["L"],) * 3)
    return z.astype(np.int64), z, z.copy(), rc.lattice_of(case)[3], z.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _special_runs(name):
    case = ENSEMBLE[name]
    return run_case(case, lat0=_full_cold(case["L"])), run_case(case, power=POWERS[1], lat0=_empty(case))


def replica_runs(name, R):
    """per replica of an ensemble case: (the comparator's run, plane set).  Replica 0 terminates at once and is frozen from
    then on, replica 1 starts empty; replicas r >= 2 cycle through three (lattice, seed, plane set) combinations, so R = 70
    costs five comparator runs."""
    cold, empty = _special_runs(name)
    runs = [(cold, 0), (empty, 1)]
    for r in range(2, R):
        v = r % 3
        runs.append((stepped(name, v, v, POWERS[v % 2]), v % 2))
    return ENSEMBLE[name], runs
