"""Inputs of the thermal-boundary GPU tests (tests/test_gpu_boundary_*.py), shared with tests/test_boundary_ref_host.py, which
asserts on the comparator alone (tests/boundary_ref.py) what each of them exercises.  The fields, lattices and calls are those
of tests/implicit_cases.py; this file adds the boundaries.

Sizes of the direct calls: the seams of csrc/thermal_imp.hpp that the end addends meet.  k_imp_lines issues its loads U = 8
elements ahead from element 1 on, so m = L - 1 falls in the last slot of a group at L = 9, the first at L = 10, a middle one at
L = 17; k_imp_rows moves chunks of 64 columns, so m = L - 1 is the last column of the only chunk at L = 64, alone in the second
at L = 65 and alone in the third at L = 129.  L = 1, 2, 3: both addends on one voxel, on neighbours, one voxel between.
"""
import functools

import numpy as np

from oracle import oracle
import boundary_ref as br
import implicit_cases as ic
import remelt_cases as rc
from substep_ref import new_stats

SIZES = (1, 2, 3, 9, 10, 17, 64, 65, 129)
SUBSTEPS = (1, 3)
DT = ic.DT
CLIP_LO, CLIP_HI = ic.CLIP_LO, ic.CLIP_HI

# six different beta between 0.37 and 2.5; T_ext inside (3300, 3900), below (1500, 2000) and above (5000, 4600) the clip range.
# The top face is a cold one: under the direct calls' source a small lattice's top plane lies on T_clip_hi with or without a hot
# face above it, and the clip would hide that face.  The i faces, solved last, balance inside the clip range, so the one voxel
# of L = 1 ends there too.
ALL_SIX = br.boundary(beta=(1.0, 0.37, 0.5, 2.5, 1.3, 0.8), T_ext=(3900.0, 1500.0, 5000.0, 3300.0, 4600.0, 2000.0))
# exactly one face each, a fixed temperature far outside the clip range (different per face: a mix-up shows)
SINGLE = {f: br.boundary(**{f: (1.0, T)}) for f, T in zip(br.FACES, (1500.0, 5000.0, 1700.0, 4800.0, 1900.0, 4600.0))}
BOUNDARIES = dict(SINGLE, all=ALL_SIX, none=None, zero=br.boundary(T_ext=(5000.0,) * 6, ramp=(7.0,) * 6))


def face_slices(L):
    m = L - 1
    return [np.s_[0], np.s_[m], np.s_[:, 0], np.s_[:, m], np.s_[:, :, 0], np.s_[:, :, m]]


@functools.lru_cache(maxsize=None)
def direct_reference(L, n, mode, key, nonfinite=False, updates=2):
    """the comparator's field after `updates` direct updates (u = 0) of implicit_cases' direct input with BOUNDARIES[key], and
    what they exercised"""
    lat, _, _, q = ic.direct_lattice(L, nonfinite)
    stats = new_stats()
    for _ in range(updates):
        br.update(lat, n, DT, mode, q, use_latent=True, scrub=True, stats=stats, bc=BOUNDARIES[key], u=0)
    return lat.T, stats


# ---- stepping: implicit_cases' lattices and calls with a boundary -------------------------------------------------------
def _from_product(b):
    return br.boundary(b["beta"], b["T_ext"], b["ramp"])


def gradient(L, cooling_rate=0.0):
    """thermal_solver.gradient_boundary: the two fixed i faces that extend build_temperature_field's ramp"""
    import thermal_solver
    return _from_product(thermal_solver.gradient_boundary(L, cooling_rate=cooling_rate))


def sink(cooling_rate=0.0):
    """main.py's --thermal-boundary sink: a fixed T_SUB under the lattice, everything else adiabatic"""
    import thermal_solver
    return _from_product(thermal_solver.thermal_boundary(bottom=("fixed", float(oracle.T_SUB)), cooling_rate=cooling_rate))


COOLING = 2e8           # K/s: 200 K per update at dt = 1e-6 s, so a wrong update ordinal moves the face by hundreds of kelvin


def _bcase(name, base, bc, **over):
    c = dict(ic.STEPPING[base] if base in ic.STEPPING else ic.ENSEMBLE[base])
    c.update(over)
    c.update(name=name, bc=bc)
    assert c["step0"] % 20 == 0, name
    return c


def _bc_of(case):
    return case["bc"](case["L"]) if callable(case["bc"]) else case["bc"]


# thermal_mode 1 with the gradient boundary, thermal_mode 2 with the substrate sink under the moving source (with and without
# latent heat); rng_mode 0 / 1 / 2, full and incremental; n = 1 and 3; remelting at L = 40; L = 136: the deferred path; a ramp
# from step0 = 40 with calls cut at 47, 60, 61, 81 (batches 7, 13, 1, 20, 26)
STEPPING = {c["name"]: c for c in (
    _bcase("L24_laser_latent_rng0_full_n1_sink", "L24_laser_latent_rng0_full_n1", sink()),
    _bcase("L24_laser_latent_rng0_full_n3_sink", "L24_laser_latent_rng0_full_n3", sink()),
    _bcase("L24_laser_nolatent_rng1_incr_n1_sink", "L24_laser_nolatent_rng1_incr_n1", sink()),
    _bcase("L24_cet_rng1_incr_n3_gradient", "L24_cet_rng1_incr_n3", gradient),
    _bcase("L24_cet_rng1_incr_n3_ramp_step40", "L24_cet_rng1_incr_n3", lambda L: gradient(L, COOLING), step0=40),
    _bcase("L40_cet_rng2_full_n1_remelt_gradient", "L40_cet_rng2_full_n1_remelt", gradient),
    _bcase("L40_cet_rng2_full_n3_ramp", "L40_cet_rng2_full_n3", lambda L: gradient(L, COOLING)),
    _bcase("L136_laser_latent_deferred_n1_sink", "L136_laser_latent_deferred_n1", sink(COOLING)),
)}
# one boundary for all replicas: the sink with a ramp, and a convective top
ENS_BC = br.boundary(i_lo=(1.0, float(oracle.T_SUB), -50.0), i_hi=(0.4, 3000.0))
ENSEMBLE = {c["name"]: c for c in (
    _bcase("ens_L30_n1_bc", "ens_L30_n1", ENS_BC),
    _bcase("ens_L33_n3_bc", "ens_L33_n3", ENS_BC),
)}
POWERS = ic.POWERS


def run_case(case, variant=0, seed_off=0, power=60.0, lat0=None, bc="case"):
    """the comparator's run of a case, in the shape of implicit_cases.run_case; bc=None: the same run between insulated walls"""
    oracle.set_threads(case["threads"])
    try:
        lat0 = ic.lattice_of(case, variant) if lat0 is None else ic.plant(lat0)
        lat = oracle.Lattice(*lat0, impurity_c=0.1)
        st = br.Stepper(lat, case["n_sub"], case["threshold"] if case["remelt"] else None, bc=_bc_of(case) if bc == "case" else bc)
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


@functools.lru_cache(maxsize=None)
def stepped_adiabatic_first_call(name):
    """the first call of a case between insulated walls (what the boundary is compared with)"""
    case = {**STEPPING, **ENSEMBLE}[name]
    return run_case(dict(case, batches=case["batches"][:1]), bc=None)


@functools.lru_cache(maxsize=None)
def _special_runs(name):
    case = ENSEMBLE[name]
    return run_case(case, lat0=ic._full_cold(case["L"])), run_case(case, power=POWERS[1], lat0=ic._empty(case))


def replica_runs(name, R):
    """per replica: (the comparator's run, plane set), built like implicit_cases.replica_runs: replica 0 terminates at once
    and is frozen from then on, replica 1 starts empty, the others cycle through three (lattice, seed, plane set) combinations"""
    cold, empty = _special_runs(name)
    runs = [(cold, 0), (empty, 1)]
    for r in range(2, R):
        v = r % 3
        runs.append((stepped(name, v, v, POWERS[v % 2]), v % 2))
    return ENSEMBLE[name], runs
