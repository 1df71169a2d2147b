"""Inputs of the beam-table GPU tests (tests/test_gpu_beam_*.py), shared with tests/test_beam_ref_host.py, which asserts on the
comparator alone (tests/beam_ref.py) what each of them exercises.  The fields, lattices and calls are those of
tests/implicit_cases.py; this file adds the tables.

The beam radius is 1.5 voxels: with the cutoff of 3 radii that leaves 9 non-zero factors per axis, so a lattice of 24 holds rows
inside and outside the footprint.  Power: the peak of the source is amp dt / rho_cp = 155 K per watt and update at depth 1
before the solves spread it (amp = P a / (pi r_b^2) / dx, r_b = 7.5e-6 m, dx = 5e-6 m, rho_cp = 2.5476e6 J/m^3-K, dt = 1e-6 s),
44 times what a watt does at the default radius of 10 voxels.  The direct calls use 1.5 W on implicit_cases' rough field (whose
solves pull every voxel towards 3400 K), the stepping calls 1.4 W (the 210 K per update of implicit_cases' 60 W planes): the
heated voxels stay off T_clip_hi (tests/test_beam_ref_host.py asserts it).

Sizes of the direct calls: 1, 2, 3, 5 and 9 (one partial block of 64 rows up to a few), 63 / 64 / 65 (the beam's centre three
voxels inside the far corner puts the footprint's edge and the depth boundary inside, on and across a 64-row block and a
64-column chunk of k_imp_rows), 129 (the third chunk), and 256 once.
"""
import functools

import numpy as np

from oracle import oracle
import beam_ref
import boundary_cases as bcs
import implicit_cases as ic
import remelt_cases as rc
from substep_ref import new_stats

SIZES = (1, 2, 3, 5, 9, 63, 64, 65, 129)
DT = ic.DT
RADIUS = 1.5 * oracle.VOXEL_SIZE
U0 = 5                      # the direct tables begin at update ordinal 5: rows 0 and 1 on, row 2 off
POWER_DIRECT, POWER_STEP = 1.5, 1.4
PENETRATION = 2.0 * oracle.VOXEL_SIZE


def depths(L):
    return sorted({d for d in (1, 2, L) if d <= L})


def _centres(L):
    """row 0: three voxels inside the far corner; row 1: near the j = 0 edge, mid k; row 2: off"""
    m = L - 1
    return ((m - 3.2, m - 3.2, True), (min(2.3, m), m / 2.0 + 0.4, True), (m / 2.0, m / 2.0, False))


@functools.lru_cache(maxsize=None)
def direct_table(L, D):
    import thermal_solver
    c = _centres(L)
    return thermal_solver.beam_table(L, lambda u: c[u - U0], U0, 3, POWER_DIRECT, beam_radius=RADIUS, absorptivity=0.35, depth=D,
                                     penetration=None if D <= 2 else PENETRATION)


# (L, D, n, latent): every size and fitting depth with n = 1 with and without latent heat, and n = 3 with it
DIRECT = [(L, D, n, lat) for L in SIZES for D in depths(L) for (n, lat) in ((1, True), (1, False), (3, True))]


@functools.lru_cache(maxsize=None)
def direct_reference(L, D, n, latent=True, key="none", nonfinite=False, ordinals=(U0, U0 + 1)):
    """the comparator's field after the updates `ordinals` of implicit_cases' direct input from direct_table(L, D) with
    boundary_cases.BOUNDARIES[key], and what they exercised"""
    lat, _, _, _ = ic.direct_lattice(L, nonfinite)
    stats = new_stats()
    heated_max = -np.inf
    t = direct_table(L, D)
    for u in ordinals:
        beam_ref.update(lat, n, DT, t, u, use_latent=latent, scrub=True, stats=stats, bc=bcs.BOUNDARIES[key])
        hot = beam_ref.source(t, L, u - U0) != 0.0
        if hot.any():
            heated_max = max(heated_max, float(lat.T[hot].max()))
    stats["heated_max"] = heated_max
    return lat.T, stats


def nonfinite_in_footprint(L, D):
    """implicit_cases' direct field with a NaN and a +inf on heated voxels of row 0's footprint"""
    t = direct_table(L, D)
    hot = np.argwhere(beam_ref.source(t, L, 0) != 0.0)
    T = ic.direct_fields(L)[0][3].copy()
    T[tuple(hot[0])], T[tuple(hot[-1])] = np.nan, np.inf
    return T


@functools.lru_cache(maxsize=None)
def nonfinite_reference(L, D, n):
    fields, prev, _ = ic.direct_fields(L)
    lat = oracle.Lattice(fields[0], fields[1], fields[2], nonfinite_in_footprint(L, D), fields[4], impurity_c=0.1)
    lat.prev_state = np.ascontiguousarray(prev, np.int8)
    stats = new_stats()
    beam_ref.update(lat, n, DT, direct_table(L, D), U0, use_latent=True, scrub=True, stats=stats)
    return lat.T, stats


# ---- stepping: implicit_cases' lattices and calls, the source a serpentine scan --------------------------------------------
def scan_table(L, u0, n_u, D, power=POWER_STEP):
    """a serpentine scan of two updates per track (speed = the track's length), so that the second track begins at update 2:
    inside every run below.  Tracks a quarter of the lattice apart from j = L / 3."""
    import thermal_solver
    margin = L // 6
    length = L - 1 - 2.0 * margin
    path = thermal_solver.scan_path(L, "serpentine", speed=length / 1.5, hatch=L / 4.0, start=L / 3.0, margin=margin)
    return thermal_solver.beam_table(L, path, u0, n_u, power, beam_radius=RADIUS, absorptivity=0.35, depth=D,
                                     penetration=None if D <= 2 else PENETRATION)


def _bcase(name, base, D, bc=None, **over):
    c = dict(ic.STEPPING[base] if base in ic.STEPPING else ic.ENSEMBLE[base])
    c.update(over)
    c.update(name=name, bc=bc, depth=D, thermal_mode=2)
    assert c["step0"] % 20 == 0, name
    return c


# rng_mode 0 / 1 / 2, full and incremental; n = 1 and 3; with and without latent heat; D = 1, 2 and 4; u0 > 0 (step0 = 40, the
# table from ordinal 2); remelting at L = 40; the substrate sink at L = 24 and L = 136 (the deferred path)
STEPPING = {c["name"]: c for c in (
    _bcase("L24_latent_rng0_full_n1_D2", "L24_laser_latent_rng0_full_n1", 2),
    _bcase("L24_latent_rng0_full_n3_D1_sink", "L24_laser_latent_rng0_full_n3", 1, bc=bcs.sink()),
    _bcase("L24_nolatent_rng1_incr_n1_D4", "L24_laser_nolatent_rng1_incr_n1", 4),
    _bcase("L24_latent_rng0_full_n1_D2_step40", "L24_laser_latent_rng0_full_n1", 2, step0=40),
    _bcase("L40_rng2_full_n1_remelt_D2", "L40_cet_rng2_full_n1_remelt", 2),
    _bcase("L136_latent_deferred_n1_D2_sink", "L136_laser_latent_deferred_n1", 2, bc=bcs.sink(bcs.COOLING)),
)}
ENSEMBLE = {c["name"]: c for c in (
    _bcase("ens_L30_n1_D2", "ens_L30_n1", 2),
    _bcase("ens_L33_n3_D3", "ens_L33_n3", 3),
)}
ENS_POWERS = (1.4, 1.0, 1.8)         # the tables of the ensemble cases: one per power


def table_of(case, power=POWER_STEP):
    u0 = case["step0"] // 20
    n_u = (case["step0"] + sum(case["batches"]) + 19) // 20 - u0
    return scan_table(case["L"], u0, max(n_u, 1), case["depth"], power)


def calls_of(case):
    """implicit_cases' calls without their planes"""
    return [(s0, n, up, ud, unp, None) for (s0, n, up, ud, unp, _q) in rc.calls_of(dict(case, thermal_mode=1))]


def run_case(case, variant=0, seed_off=0, power=POWER_STEP, lat0=None, calls=None):
    """the comparator's run of a case, in the shape of implicit_cases.run_case"""
    oracle.set_threads(case["threads"])
    try:
        lat0 = ic.lattice_of(case, variant) if lat0 is None else ic.plant(lat0)
        lat = oracle.Lattice(*lat0, impurity_c=0.1)
        st = beam_ref.Stepper(lat, table_of(case, power), case["n_sub"], case["threshold"] if case["remelt"] else None, bc=case["bc"])
        calls, results, fields, nucs = calls_of(case) if calls is None else calls, [], [], []
        for (s0, n, up, ud, unp, _q) in calls:
            results.append(st.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"] + seed_off,
                                        thermal_mode=2, q_planes=None, use_latent=case["use_latent"]))
            fields.append(tuple(a.copy() for a in (lat.state, lat.theta, lat.phi, lat.T, lat.prev_state)))
            nucs.append(lat.nuc_count)
            if results[-1]["status"]:
                break
        return dict(lat0=lat0, calls=calls, results=results, fields=fields, nucs=nucs, stepper=st)
    finally:
        oracle.set_threads(1)


@functools.lru_cache(maxsize=None)
def stepped(name, variant=0, seed_off=0, power=POWER_STEP):
    return run_case({**STEPPING, **ENSEMBLE}[name], variant, seed_off, power)


@functools.lru_cache(maxsize=None)
def _special_runs(name):
    case = ENSEMBLE[name]
    return run_case(case, lat0=ic._full_cold(case["L"])), run_case(case, power=ENS_POWERS[1], lat0=ic._empty(case))


def replica_runs(name, R, n_sets):
    """per replica: (the comparator's run, table index), built like implicit_cases.replica_runs: replica 0 terminates at once
    and is frozen from then on, replica 1 starts empty, the others cycle through three (lattice, seed) combinations and the
    n_sets tables"""
    cold, empty = _special_runs(name)
    runs = [(cold, 0), (empty, 1)]
    for r in range(2, R):
        v, s = r % 3, r % n_sets
        runs.append((stepped(name, v, v, ENS_POWERS[s]), s))
    return ENSEMBLE[name], runs
