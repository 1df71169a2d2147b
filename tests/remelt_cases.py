"""Inputs of the remelting GPU tests (tests/test_gpu_remelt_*.py), shared with tests/test_remelt_ref_host.py, which asserts on
the comparator alone (tests/remelt_ref.py) that every one of them exercises what the tests are about: voxels melt at two or
more different updates, a melted voxel is refilled later, and among the melted voxels there is a listed one (an atom with an
empty neighbour), an interior one (no empty neighbour) and a state-4 one.

A case is built once per process (``stepped``): the lattice, its calls and the comparator's results after every call.
"""
import functools

import numpy as np

from oracle import oracle
from remelt_ref import Stepper

T_MELT = float(oracle.T_MELT)


def block_lattice(L, seed, t_lo=3000.0, t_hi=4000.0, sparse=0.04, smooth=False):
    """A dense block of atoms (a few state-4 voxels among them) from the top plane down, in a sparsely occupied lattice.  Beside
    the block the top plane is partly empty (deposition candidates).  T: uniform in [t_lo, t_hi) per voxel, or (smooth, the
    laser cases) rising linearly with the plane from t_lo to t_hi plus a millikelvin of noise -- the explicit update is
    unstable at the reference's dt, so a rough field is at the clip values after one update, a smooth one only where the beam
    has been; and an EMPTY top-plane voxel between about 3900 K and 3925 K has a deposition rate near the largest double, a
    few of which overflow the total: the smooth cases stay below that until the field has roughened."""
    rs = np.random.RandomState(seed)
    state = np.zeros((L, L, L), np.int64)
    occ = rs.random_sample((L, L, L)) < sparse
    species = rs.choice([1, 2, 3, 4], size=(L, L, L), p=[0.6, 0.15, 0.2, 0.05])
    state[occ] = species[occ]
    d = min(8, max(L // 3, 1))
    a, b = L // 5, L - L // 5
    blk = np.zeros((L, L, L), bool)
    top = rs.random_sample((L, L)) < 0.3
    state[L - 1][top] = species[L - 1][top]
    blk[L - 1 - d:L, a:b, a:b] = True
    state[blk] = species[blk]                                   # dense: every voxel of the block occupied
    atoms = (state >= 1) & (state <= 3)
    theta = np.where(atoms, rs.uniform(0, np.pi, (L, L, L)), 0.0)
    phi = np.where(atoms, rs.uniform(0, 2 * np.pi, (L, L, L)), 0.0)
    T = rs.uniform(t_lo, t_hi, (L, L, L))
    if smooth:
        T = t_lo + (t_hi - t_lo) * np.arange(L)[:, None, None] / max(L - 1, 1) + 1e-3 * (T - t_lo) / (t_hi - t_lo)
    defects = ((state == 3) & (rs.random_sample((L, L, L)) < 0.3)).astype(np.int64)
    return state, theta, phi, T, defects


def scan_planes(L, n, first=0, power=60.0):
    """source planes first .. first + n - 1 of a scan: the beam (oracle.laser_source_plane; 60 W heat its centre by about
    210 K per update) moves by a third of the lattice per update, so that every update melts fresh material"""
    return np.stack([oracle.laser_source_plane(L, (L - 1, (L / 4.0 + (L / 3.0) * u) % L), power) for u in range(first, first + n)])


def calls_of(case, power=60.0):
    """(step0, n, u_pick, u_defect, u_np, q_planes) per call, back to back from case['step0']; u_np covers rng_mode 0's worst
    case (L^2 deposition candidates + two orientation draws a step) or rng_mode 1's two draws a step"""
    L, out, s, u = case["L"], [], case["step0"], 0
    for k, n in enumerate(case["batches"]):
        rs = np.random.RandomState(case["seed"] * 1000 + k)
        n_np = n * (L * L + 2) if case["rng_mode"] == 0 else 2 * n + 2
        n_q = sum(1 for g in range(s, s + n) if g % 20 == 0)
        q = scan_planes(L, n_q + 1, first=u, power=power) if case["thermal_mode"] == 2 else None
        out.append((s, n, rs.random_sample(n), rs.random_sample(n), rs.random_sample(n_np), q))
        s, u = s + n, u + n_q
    return out


def _case(name, L, seed, thermal_mode, threshold, batches, step0=0, rng_mode=1, use_latent=True, incremental=False,
          defect_fraction=0.0, threads=1, **lat):
    return dict(name=name, L=L, seed=seed, thermal_mode=thermal_mode, threshold=threshold, batches=tuple(batches), step0=step0,
                rng_mode=rng_mode, use_latent=use_latent, incremental=incremental, defect_fraction=defect_fraction,
                threads=threads, lat=lat)


# thermal_mode 1 has no source: the threshold is lowered into the range the field spans.  3300.125 and T_MELT are far from the
# clip values 2800 and 4064.5, which many voxels hold exactly after an update.
STEPPING = {c["name"]: c for c in (
    _case("L24_laser_latent_rng0_full", 24, 1, 2, T_MELT, (7, 13, 1, 20, 26), rng_mode=0, defect_fraction=0.1, smooth=True, t_lo=3500.0, t_hi=3650.0),
    _case("L24_laser_nolatent_rng1_incr", 24, 2, 2, T_MELT, (7, 13, 1, 20, 26), use_latent=False, incremental=True, defect_fraction=0.05, smooth=True, t_lo=3500.0, t_hi=3650.0),
    _case("L40_cet_lowered_rng2_full", 40, 3, 1, 3300.125, (21, 20, 5), rng_mode=2),
    _case("L64_laser_latent_rng1_incr", 64, 4, 2, T_MELT, (21, 20, 5), incremental=True, defect_fraction=0.1, smooth=True, t_lo=3500.0, t_hi=3650.0),
    _case("L136_laser_latent_deferred", 136, 5, 2, T_MELT, (19, 3, 21), step0=1, threads=16, smooth=True, t_lo=3500.0, t_hi=3650.0),
    _case("L256_fused_tiles", 256, 6, 2, T_MELT, (23,), step0=19, threads=16, smooth=True, t_lo=3500.0, t_hi=3650.0),
)}
ENSEMBLE = {c["name"]: c for c in (
    _case("ens_L30", 30, 11, 2, T_MELT, (23, 20), step0=19, rng_mode=0, defect_fraction=0.05, smooth=True, t_lo=3500.0, t_hi=3650.0),
    _case("ens_L33", 33, 12, 2, T_MELT, (12, 11), step0=19, rng_mode=2, smooth=True, t_lo=3500.0, t_hi=3650.0),
)}


def lattice_of(case, variant=0):
    return block_lattice(case["L"], case["seed"] + 100 * variant, **case["lat"])


def run_case(case, variant=0, seed_off=0, power=60.0, lat0=None):
    """The comparator's run of a case (variant: which lattice; seed_off: added to the rng_mode 2 seed; power: of the source
    planes; lat0: a lattice of the caller's instead): dict(lat0 = the initial fields, calls, results = its result after every call, fields =
    (state, theta, phi, T, prev_state) after every call, info and nucleation count after every call, stepper)."""
    oracle.set_threads(case["threads"])
    try:
        lat0 = lattice_of(case, variant) if lat0 is None else lat0
        lat = oracle.Lattice(*lat0, impurity_c=0.1)
        st = Stepper(lat, case["threshold"])
        calls, results, fields, infos, nucs = calls_of(case, power), [], [], [], []
        for (s0, n, up, ud, unp, q) in calls:
            results.append(st.run_steps(s0, n, case["defect_fraction"], up, ud, unp, rng_mode=case["rng_mode"], seed=case["seed"] + seed_off,
                                        thermal_mode=case["thermal_mode"], q_planes=q, use_latent=case["use_latent"]))
            fields.append(tuple(a.copy() for a in (lat.state, lat.theta, lat.phi, lat.T, lat.prev_state)))
            infos.append(dict(st.info))
            nucs.append(lat.nuc_count)
            if results[-1]["status"]:
                break
        return dict(lat0=lat0, calls=calls, results=results, fields=fields, infos=infos, nucs=nucs, stepper=st)
    finally:
        oracle.set_threads(1)


@functools.lru_cache(maxsize=None)
def stepped(name, variant=0, seed_off=0, power=60.0):
    return run_case({**STEPPING, **ENSEMBLE}[name], variant, seed_off, power)


class LatView:
    """the comparator's lattice after call c of a run, as helpers.assert_call_matches_oracle reads an oracle lattice"""

    def __init__(self, run, c, impurity_c=0.1):
        st, th, ph, T, _prev = run["fields"][c]
        lat = oracle.Lattice(st, th, ph, T, run["lat0"][4], impurity_c=impurity_c)
        self.state, self.theta, self.phi, self.T, self.defects = st, th, ph, T, lat.defects
        self.sweep, self.nuc_count = lat.sweep, run["nucs"][c]


# ---- the direct call (tests/test_gpu_remelt_call.py) ------------------------------------------------------------------
DIRECT_SIZES = (1, 2, 3, 5, 33, 64, 65, 129, 264)
DIRECT_KINDS = ("crafted", "plane", "all", "nothing")


@functools.lru_cache(maxsize=2)
def _direct_base(L):
    """(state: 60 % occupied, one voxel in sixteen of those a state-4 one; T below the threshold; a uniform per voxel for the
    orientations) -- built once per size"""
    rs = np.random.RandomState(1000 + L)
    u = rs.randint(0, 160, (L, L, L))
    state = np.where(u < 64, 0, np.where(u < 120, 1, np.where(u < 134, 2, np.where(u < 154, 3, 4)))).astype(np.int64)
    return state, rs.uniform(2900.0, 3600.0, (L, L, L)), rs.random_sample((L, L, L))


def direct_case(L, kind):
    """((state, theta, phi, T, defects), threshold, claim) with claim = dict(melts = voxels that must melt, stays = voxels that
    must not).  A dense random lattice with every temperature below the threshold, then, by kind:
      crafted  the eight corners, the edge (0, 0, k), a face centre, an interior voxel, k-runs across 7/8/9 and 63/64/65 and the
               last voxel of a row made hot; one atom exactly on the threshold and one at +inf (melt), one an ulp below and one
               at NaN (stay); hot EMPTY voxels with an orientation (stay);
      plane    plane L // 2 hot;  all: everything hot;  nothing: as it is."""
    rs = np.random.RandomState(1000 + L)
    state, T, ang = (a.copy() for a in _direct_base(L))
    thr, hot = T_MELT, T_MELT + 100.0
    melts, stays = set(), set()
    if kind == "crafted":
        m = L - 1
        named = [(a, b, c) for a in (0, m) for b in (0, m) for c in (0, m)]                   # corners
        named += [(0, 0, k) for k in range(L)]                                                # an edge
        named += [(0, L // 2, L // 2), (L // 2, L // 2, L // 2)]                              # face centre, interior
        named += [(L // 2, L // 3, k) for k in (7, 8, 9, 63, 64, 65, m) if k < L]             # k-runs, the row's last voxel
        for q, v in enumerate(named):
            state[v] = 1 + q % 4                 # every fourth one a state-4 voxel
            T[v] = hot
        melts |= set(named)
        special = [(L // 3, L // 2, k) for k in range(4) if k < L]
        for v, (t, goes) in zip(special, ((thr, True), (np.nextafter(thr, -np.inf), False), (np.nan, False), (np.inf, True))):
            if v in melts:
                continue                          # (tiny lattices: the voxel is already one of the named ones)
            state[v] = 1 + (v[2] % 3)
            T[v] = t
            (melts if goes else stays).add(v)
        for k in range(min(L, 5)):
            v = (L // 3, L // 3, k)
            if v not in melts and v not in stays:
                state[v] = 0
                T[v] = hot
                stays.add(v)
    elif kind == "plane":
        T[L // 2] = hot
    elif kind == "all":
        T[:] = hot
    atoms = (state >= 1) & (state <= 3)
    theta = np.where(atoms, np.pi * ang, 0.0)
    phi = np.where(atoms, 2 * np.pi * (1.0 - ang), 0.0)
    for v in stays:
        if state[v] == 0:
            theta[v], phi[v] = 1.0, 2.0          # an empty voxel's orientation is kept
    defects = ((state == 3) & (rs.random_sample((L, L, L)) < 0.3)).astype(np.int64)
    return (state, theta, phi, T, defects), thr, dict(melts=melts, stays=stays)
