"""Microstructure metrics (drop-in for the reference ``metrics.py``; host-side NumPy).

``compute_metrics`` returns the same 17-key dict (metrics.py:41-96) including the reference's
quirk that the grain-diameter percentiles are taken over the LABEL volume returned by
``get_clusters`` (metrics.py:43,76 <-> utils.py:84).
"""
import numpy as np

from constants import CET_AR_THRESHOLD, CET_EQ_THRESHOLD, T_MELT, VOXEL_SIZE
from utils import calculate_aspect_ratio, get_clusters


def grain_aspect_ratio(state, voxel_size=VOXEL_SIZE):
    """Height (axis 2) over the larger lateral extent of the occupied region (metrics.py:6-15)."""
    occ = np.argwhere(state > 0)
    if occ.size == 0:
        return 0.0
    ext = occ.max(axis=0) - occ.min(axis=0) + 1
    return (ext[2] * voxel_size) / (max(ext[0], ext[1]) * voxel_size + 1e-12)


def equiaxed_fraction(state, threshold=CET_AR_THRESHOLD, voxel_size=VOXEL_SIZE):
    if np.argwhere(state > 0).size == 0:
        return 0.0
    return 1.0 if grain_aspect_ratio(state, voxel_size) < threshold else 0.0


def nucleation_density(state, voxel_size=VOXEL_SIZE):
    volume = np.prod(state.shape) * (voxel_size ** 3)
    return np.count_nonzero(state > 0) / volume if volume > 0 else 0.0


def grain_sizes(state):
    occ = np.argwhere(state > 0)
    return [] if occ.size == 0 else [len(occ)]


def compute_voxel_fraction(count, total_voxels):
    return count / total_voxels if total_voxels > 0 else 0.0


def compute_boundary_fraction(impurity_mask, grain_ids):
    """Fraction of flagged voxels with a 6-neighbour of a different grain id, edges replicated
    (metrics.py:113-138)."""
    n_imp = np.count_nonzero(impurity_mask)
    if n_imp == 0:
        return 0.0
    g = np.pad(grain_ids, 1, mode="edge")
    core = g[1:-1, 1:-1, 1:-1]
    differs = np.zeros(grain_ids.shape, dtype=bool)
    for sl in ((slice(2, None), slice(1, -1), slice(1, -1)), (slice(None, -2), slice(1, -1), slice(1, -1)),
               (slice(1, -1), slice(2, None), slice(1, -1)), (slice(1, -1), slice(None, -2), slice(1, -1)),
               (slice(1, -1), slice(1, -1), slice(2, None)), (slice(1, -1), slice(1, -1), slice(None, -2))):
        differs |= g[sl] != core
    return np.count_nonzero(differs & np.asarray(impurity_mask, dtype=bool)) / n_imp


def equivalent_diameter_um(cluster_sizes, voxel_size):
    """(d50, d90) in micrometres of sphere-equivalent diameters (metrics.py:141-150)."""
    if len(cluster_sizes) == 0:
        return 0.0, 0.0
    volumes = np.array(cluster_sizes) * (voxel_size ** 3)
    d = ((6.0 * volumes / np.pi) ** (1.0 / 3.0)) * 1e6
    return np.median(d), np.percentile(d, 90)


def compute_metrics(state, theta, phi, defects=None, voxel_size=VOXEL_SIZE,
                    W_mask=None, Re_mask=None, C_mask=None, grain_ids=None, rng_seed=None):
    clusters, label_volume = get_clusters(state, theta, phi, theta_threshold=0.5)
    if not clusters:
        return {
            "AspectRatio": 0.0, "EquiaxedFraction": 0.0, "NucleationDensity": 0.0,
            "AvgGrainSize": 0.0, "GrainCount": 0, "DefectDensity": 0.0,
            "Frac_W": 0.0, "Frac_Re": 0.0, "Frac_C": 0.0,
            "C_boundary_frac": 0.0, "Re_boundary_frac": 0.0,
            "Defect_voxel_count": 0, "Defect_voxel_frac": 0.0,
            "Grain_d50_um": 0.0, "Grain_d90_um": 0.0,
            "VOXEL_SIZE_m": voxel_size, "RANDOM_SEED": rng_seed,
        }
    ars = [calculate_aspect_ratio(c) for c in clusters]
    volume = state.size * (voxel_size ** 3)
    n_vox = state.size
    n_def = np.sum(defects) if defects is not None else 0
    d50, d90 = equivalent_diameter_um(label_volume, voxel_size)

    def frac(mask):
        return compute_voxel_fraction(np.count_nonzero(mask), n_vox) if mask is not None else 0.0

    def bfrac(mask):
        return compute_boundary_fraction(mask, grain_ids) if (mask is not None and grain_ids is not None) else 0.0

    return {
        "AspectRatio": np.mean(ars),
        "EquiaxedFraction": np.mean(np.array(ars) < CET_AR_THRESHOLD),
        "NucleationDensity": len(clusters) / volume if volume > 0 else 0.0,
        "AvgGrainSize": np.mean([len(c) for c in clusters]) * voxel_size * 1e6,
        "GrainCount": len(clusters),
        "DefectDensity": n_def / volume if volume > 0 else 0.0,
        "Frac_W": frac(W_mask), "Frac_Re": frac(Re_mask), "Frac_C": frac(C_mask),
        "C_boundary_frac": bfrac(C_mask), "Re_boundary_frac": bfrac(Re_mask),
        "Defect_voxel_count": n_def,
        "Defect_voxel_frac": compute_voxel_fraction(n_def, n_vox),
        "Grain_d50_um": d50, "Grain_d90_um": d90,
        "VOXEL_SIZE_m": voxel_size, "RANDOM_SEED": rng_seed,
    }


def compute_metrics_device(engine, n_voxels, defects_count=0, voxel_size=VOXEL_SIZE, rng_seed=None):
    """Same dict as :func:`compute_metrics` (without the optional mask fractions), but the grain
    clustering runs on the GPU on the lattice resident in ``engine`` (cetkmc_cluster: connected
    components, numbered like the reference's DFS, utils.py:28-84).  Only the per-cluster sizes /
    bounding boxes and the int32 label volume (for the d50/d90 quirk, metrics.py:76) cross PCIe."""
    return compute_metrics_from_clusters(engine.clusters(0.5, labels=True), n_voxels, defects_count, voxel_size, rng_seed)


def compute_metrics_from_clusters(cl, n_voxels, defects_count=0, voxel_size=VOXEL_SIZE, rng_seed=None):
    """compute_metrics_device's dict from an already computed clustering (Engine.clusters(0.5, labels=True) or one
    replica's entry of Ensemble.analyze)."""
    n = len(cl["size"])
    if n == 0:
        return {
            "AspectRatio": 0.0, "EquiaxedFraction": 0.0, "NucleationDensity": 0.0,
            "AvgGrainSize": 0.0, "GrainCount": 0, "DefectDensity": 0.0,
            "Frac_W": 0.0, "Frac_Re": 0.0, "Frac_C": 0.0,
            "C_boundary_frac": 0.0, "Re_boundary_frac": 0.0,
            "Defect_voxel_count": 0, "Defect_voxel_frac": 0.0,
            "Grain_d50_um": 0.0, "Grain_d90_um": 0.0,
            "VOXEL_SIZE_m": voxel_size, "RANDOM_SEED": rng_seed,
        }
    dims = (cl["bbox"][:, 3:6] - cl["bbox"][:, 0:3] + 1).astype(np.int64)
    ars = [float(lo_hi[1]) / float(max(lo_hi[0], 1)) for lo_hi in zip(dims.min(axis=1).tolist(), dims.max(axis=1).tolist())]
    sizes = cl["size"].tolist()
    volume = n_voxels * (voxel_size ** 3)
    d50, d90 = equivalent_diameter_um(cl["labels"], voxel_size)
    return {
        "AspectRatio": np.mean(ars),
        "EquiaxedFraction": np.mean(np.array(ars) < CET_AR_THRESHOLD),
        "NucleationDensity": n / volume if volume > 0 else 0.0,
        "AvgGrainSize": np.mean(sizes) * voxel_size * 1e6,
        "GrainCount": n,
        "DefectDensity": defects_count / volume if volume > 0 else 0.0,
        "Frac_W": 0.0, "Frac_Re": 0.0, "Frac_C": 0.0,
        "C_boundary_frac": 0.0, "Re_boundary_frac": 0.0,
        "Defect_voxel_count": defects_count,
        "Defect_voxel_frac": compute_voxel_fraction(defects_count, n_voxels),
        "Grain_d50_um": d50, "Grain_d90_um": d90,
        "VOXEL_SIZE_m": voxel_size, "RANDOM_SEED": rng_seed,
    }


FRONT_COLUMNS = ("G_front", "G_front_max", "Gi_front", "T_front", "Undercooling_front", "Front_i", "FrontVoxels",
                 "MeltVoxels", "MeltDepth", "MeltLength", "MeltWidth")


def front_metrics(stats, L, voxel_size=VOXEL_SIZE):
    """Columns of a metrics row from one lattice's front statistics (Engine.front_stats, or entry r of every array of
    Ensemble.front_stats; taken with inv_dx = 1 / voxel_size, so gradients are in K/m): G_front (mean |grad T| over the
    front voxels), G_front_max, Gi_front (mean component along the build direction), T_front (mean), Undercooling_front
    (T_MELT - T_front), Front_i (mean plane index of the front), FrontVoxels (n_front: 0 marks a row without a front),
    MeltVoxels and MeltDepth / MeltLength / MeltWidth (extents of the melt voxels' bounding box along i, j, k in voxels).
    Everything that is a mean over an empty front (Undercooling_front included) is 0.0; the extents of an empty pool are 0."""
    n = int(stats["n_front"])
    bb = [int(x) for x in stats["melt_bbox"]]
    n_melt = int(stats["n_melt"])
    mean = (lambda x: float(x) / n) if n else (lambda x: 0.0)
    T_front = mean(stats["T_sum"])
    ext = [(bb[3 + a] - bb[a] + 1) if n_melt else 0 for a in range(3)]
    return {
        "G_front": mean(stats["G_sum"]), "G_front_max": float(stats["G_max"]) if n else 0.0, "Gi_front": mean(stats["Gi_sum"]),
        "T_front": T_front, "Undercooling_front": (float(T_MELT) - T_front) if n else 0.0,
        "Front_i": mean(int(stats["pos_sum"][0])), "FrontVoxels": n,
        "MeltVoxels": n_melt, "MeltDepth": ext[0], "MeltLength": ext[1], "MeltWidth": ext[2],
    }


LAYER_COLUMNS = ("CET_plane", "CET_height_um", "EqAreaFrac", "Intercept_build_um", "Intercept_plane_um", "InterceptRatio",
                 "GB_frac_W", "GB_frac_Re", "GB_frac_C")


def layer_metrics(profile, L, voxel_size=VOXEL_SIZE):
    """Columns of a metrics row (LAYER_COLUMNS) from one lattice's layer profile (Engine.layer_profile, or entry r of every
    array of Ensemble.layer_profile), plus the per-plane arrays under "planes" (the rows of layers.csv).

    EqAreaFrac: voxels of equiaxed grains over occupied voxels.  CET_plane: the lowest occupied plane from which on every
    occupied plane has more than CET_EQ_THRESHOLD of its occupied voxels in equiaxed grains (-1: none); CET_height_um its
    height (-1.0: none).  Intercept_build_um / Intercept_plane_um: mean intercept length (occupied voxels per grain
    segment of the test lines) along the build direction / averaged over the two in-plane axes; InterceptRatio build over
    plane (> 1: elongated along the build direction).  GB_frac_W / _Re / _C: of the voxels of that species, the fraction
    with a face neighbour in another grain or empty (metrics.compute_boundary_fraction with grain_ids = labels).  Every
    ratio with a zero denominator is 0.0."""
    n_occ = np.asarray(profile["n_occ"], dtype=np.int64).reshape(L)
    n_eq = np.asarray(profile["n_eq"], dtype=np.int64).reshape(L)
    seg = np.asarray(profile["seg"], dtype=np.int64).reshape(L, 3)
    occ_state = np.asarray(profile["occ_state"], dtype=np.int64).reshape(L, 4)
    gb_state = np.asarray(profile["gb_state"], dtype=np.int64).reshape(L, 4)

    def ratio(a, b):
        return float(a) / float(b) if b else 0.0

    tot = int(n_occ.sum())
    cet = -1
    for i in range(L - 1, -1, -1):              # downwards from the top: the run of equiaxed planes that reaches it
        if n_occ[i] == 0:
            continue
        if ratio(n_eq[i], n_occ[i]) > CET_EQ_THRESHOLD:
            cet = i
        else:
            break
    build = ratio(tot, int(seg[:, 0].sum())) * voxel_size * 1e6
    plane = ratio(2 * tot, int(seg[:, 1].sum() + seg[:, 2].sum())) * voxel_size * 1e6
    occ_t, gb_t = occ_state.sum(axis=0), gb_state.sum(axis=0)
    out = {
        "CET_plane": cet, "CET_height_um": cet * voxel_size * 1e6 if cet >= 0 else -1.0,
        "EqAreaFrac": ratio(int(n_eq.sum()), tot),
        "Intercept_build_um": build, "Intercept_plane_um": plane, "InterceptRatio": ratio(build, plane),
        "GB_frac_W": ratio(gb_t[0], occ_t[0]), "GB_frac_Re": ratio(gb_t[1], occ_t[1]), "GB_frac_C": ratio(gb_t[2], occ_t[2]),
    }
    planes = {"plane": np.arange(L, dtype=np.int64), "n_occ": n_occ,
              "n_start": np.asarray(profile["n_start"], dtype=np.int64).reshape(L), "n_eq": n_eq,
              "EqAreaFrac_i": np.array([ratio(a, b) for a, b in zip(n_eq.tolist(), n_occ.tolist())], dtype=np.float64)}
    cut = np.asarray(profile["cut"], dtype=np.int64).reshape(L, 3)
    for a in range(3):
        planes[f"seg{a}"] = seg[:, a]
    for a in range(3):
        planes[f"cut{a}"] = cut[:, a]
    for t, name in enumerate(("W", "Re", "C", "defect")):
        planes[f"occ_{name}"] = occ_state[:, t]
        planes[f"gb_{name}"] = gb_state[:, t]
    out["planes"] = planes
    return out


def write_layers_csv(path, planes):
    """The per-plane table of :func:`layer_metrics` (its "planes" entry) as a CSV with one row per plane."""
    import csv
    names = list(planes)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(names)
        for i in range(len(planes["plane"])):
            w.writerow([planes[n][i].item() for n in names])


TEXTURE_COLUMNS = ("GB_faces", "GB_misorientation_mean_deg", "GB_low_angle_frac", "GB_lateral_frac", "Pole_aligned_frac",
                   "Texture_bad")
TEXTURE_LOW_ANGLE_DEG = 15.0


def texture_metrics(profile, low_angle_deg=TEXTURE_LOW_ANGLE_DEG):
    """Columns of a metrics row (TEXTURE_COLUMNS) from one lattice's texture profile (Engine.texture_profile, or entry r of
    the three count arrays of Ensemble.texture_profile with the edge angles beside them), plus the per-plane table under
    "planes" (the rows of texture.csv).  Everything is computed here, on the host, from the integer bins.

    GB_faces: grain-grain faces that fell into a bin.  GB_misorientation_mean_deg: their mean misorientation with every
    face at the centre of its bin (the bins span 0..180 degrees between the interior edges).  GB_low_angle_frac: the share
    of them in bins that end at or below ``low_angle_deg`` (the default 5-degree edges contain 15 degrees; with other edges
    a bin that straddles the angle is not counted).  GB_lateral_frac: the share across lattice axes 1 and 2, i.e. of
    boundaries that run along the build direction.  Pole_aligned_frac: of the binned voxels, the share within
    ``low_angle_deg`` of the axis (bins span 0..90 degrees).  Texture_bad: faces and voxels whose value was not finite
    (they are in no bin and in none of the ratios).  Every ratio with a zero denominator is 0.0."""
    gb = np.asarray(profile["gb_hist"], dtype=np.int64)
    pole = np.asarray(profile["pole_hist"], dtype=np.int64)
    bad = np.asarray(profile["bad"], dtype=np.int64)
    L, nb = pole.shape
    gb = gb.reshape(L, 3, nb)
    bad = bad.reshape(L, 4)
    gb_full = np.concatenate(([0.0], np.asarray(profile["gb_edges_deg"], dtype=np.float64), [180.0]))
    pole_full = np.concatenate(([0.0], np.asarray(profile["pole_edges_deg"], dtype=np.float64), [90.0]))
    gb_centre = 0.5 * (gb_full[:-1] + gb_full[1:])
    gb_low = gb_full[1:] <= low_angle_deg + 1e-9
    pole_low = pole_full[1:] <= low_angle_deg + 1e-9

    def ratio(a, b):
        return float(a) / float(b) if b else 0.0

    def columns(g, p):            # g (3, nb), p (nb,): one plane or the sum over the planes
        faces, by_bin = int(g.sum()), g.sum(axis=0)
        return (faces, ratio(float(np.dot(by_bin, gb_centre)), faces), ratio(int(by_bin[gb_low].sum()), faces),
                ratio(int(g[1].sum() + g[2].sum()), faces), ratio(int(p[pole_low].sum()), int(p.sum())))

    tot = columns(gb.sum(axis=0), pole.sum(axis=0))
    out = dict(zip(TEXTURE_COLUMNS[:5], tot))
    out["Texture_bad"] = int(bad.sum())
    per = [columns(gb[i], pole[i]) for i in range(L)]
    planes = {"plane": np.arange(L, dtype=np.int64)}
    for c, name in enumerate(TEXTURE_COLUMNS[:5]):
        planes[name] = np.array([x[c] for x in per], dtype=np.int64 if c == 0 else np.float64)
    for a in range(3):
        planes[f"GB_faces{a}"] = gb[:, a, :].sum(axis=1)
    for a in range(4):
        planes[f"bad{a}"] = bad[:, a]
    for a in range(3):
        for b in range(nb):
            planes[f"gb{a}_bin{b}"] = gb[:, a, b]
    for b in range(nb):
        planes[f"pole_bin{b}"] = pole[:, b]
    out["planes"] = planes
    return out


def write_texture_csv(path, planes):
    """The per-plane table of :func:`texture_metrics` (its "planes" entry) as a CSV with one row per plane: the summary
    columns of the plane, its faces per axis, the non-finite counts and the raw bins."""
    write_layers_csv(path, planes)


GRAIN_COLUMNS = ("Grain_elong_mean", "Columnar_vol_frac", "Grain_incl_mean_deg", "Largest_grain_frac", "Contact_same_frac",
                 "Aligned_vol_frac")


def grain_metrics(table, voxel_size=VOXEL_SIZE):
    """Columns of a metrics row (GRAIN_COLUMNS) from one lattice's per-grain table (Engine.grain_table, or one entry of
    Ensemble.grain_table), plus the per-grain table under "grains" (the rows of grains.csv).  Everything is computed here,
    on the host, in double, from the integer sums.

    Per grain: centroid c = sum / n; covariance C_ab = sq_ab / n - c_a c_b plus 1/12 on the diagonal for the voxel's own
    extent (a single voxel is isotropic, an a x b x c box has a^2/12, b^2/12, c^2/12); its eigenvalues (np.linalg.eigh) give
    the principal lengths sqrt(12 lambda) in voxels, elong = sqrt(lambda_max / lambda_min) and incl_deg, the angle between
    the major axis and the build direction (axis 0), 0..90.

    Grain_elong_mean: volume-weighted mean of elong.  Columnar_vol_frac: share of the occupied voxels in grains with elong >=
    CET_AR_THRESHOLD and incl_deg <= 45.  Grain_incl_mean_deg: volume-weighted mean of incl_deg over the grains with elong
    >= CET_AR_THRESHOLD (the inclination is read only where the major axis is well defined).  Largest_grain_frac: max n /
    sum n.  Contact_same_frac: same-grain stencil contacts over same-grain plus other-grain ones.  Aligned_vol_frac: share
    of the occupied voxels in grains whose first-voxel orientation vector lies within TEXTURE_LOW_ANGLE_DEG of the build
    axis or its opposite (a non-finite angle is not aligned).  Every ratio with a zero denominator is 0.0.  ``voxel_size``
    scales nothing here (lengths are in voxels); it is accepted like its siblings' for a uniform call."""
    n = np.asarray(table["n"], dtype=np.int64).reshape(-1)
    k = len(n)
    nf = n.astype(np.float64)
    s = np.asarray(table["sum"], dtype=np.int64).reshape(k, 3).astype(np.float64)
    q = np.asarray(table["sq"], dtype=np.int64).reshape(k, 6).astype(np.float64)
    nb = np.asarray(table["nb"], dtype=np.int64).reshape(k, 4)
    n_state = np.asarray(table["n_state"], dtype=np.int64).reshape(k, 4)
    th = np.asarray(table["first_theta"], dtype=np.float64).reshape(-1)
    ph = np.asarray(table["first_phi"], dtype=np.float64).reshape(-1)
    safe = np.maximum(nf, 1.0)[:, None]
    c = s / safe
    m = q / safe
    cov = np.zeros((k, 3, 3))
    for a, b, col in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (0, 1, 3), (0, 2, 4), (1, 2, 5)):
        cov[:, a, b] = cov[:, b, a] = m[:, col] - c[:, a] * c[:, b]
    cov[:, (0, 1, 2), (0, 1, 2)] += 1.0 / 12.0
    if k:
        lam, vec = np.linalg.eigh(cov)                  # ascending eigenvalues, eigenvectors in columns
    else:
        lam, vec = np.zeros((0, 3)), np.zeros((0, 3, 3))
    lam = np.maximum(lam, 1e-300)
    elong = np.sqrt(lam[:, 2] / lam[:, 0])
    incl = np.degrees(np.arccos(np.clip(np.abs(vec[:, 0, 2]), 0.0, 1.0)))
    with np.errstate(invalid="ignore"):
        pole = np.abs(np.sin(th) * np.cos(ph))           # |component 0| of the orientation vector: the texture profile's axis
        aligned = np.isfinite(pole) & (pole >= np.cos(np.radians(TEXTURE_LOW_ANGLE_DEG)))

    def ratio(a, b):
        return float(a) / float(b) if b else 0.0

    tot = float(nf.sum())
    col = elong >= CET_AR_THRESHOLD
    same, other = int(nb[:, 0].sum()), int(nb[:, 1].sum())
    out = {
        "Grain_elong_mean": ratio(float((nf * elong).sum()), tot),
        "Columnar_vol_frac": ratio(float(nf[col & (incl <= 45.0)].sum()), tot),
        "Grain_incl_mean_deg": ratio(float((nf * incl)[col].sum()), float(nf[col].sum())),
        "Largest_grain_frac": ratio(float(nf.max()) if k else 0.0, tot),
        "Contact_same_frac": ratio(same, same + other),
        "Aligned_vol_frac": ratio(float(nf[aligned].sum()), tot),
    }
    length = np.sqrt(12.0 * lam)
    grains = {"id": np.arange(1, k + 1, dtype=np.int64), "n": n}
    for a, name in enumerate(("ci", "cj", "ck")):
        grains[name] = c[:, a]
    for a, name in enumerate(("len_major", "len_mid", "len_minor")):
        grains[name] = length[:, 2 - a]
    grains["elong"], grains["incl_deg"] = elong, incl
    for t, name in enumerate(("W", "Re", "C", "defect")):
        grains[f"n_{name}"] = n_state[:, t]
    for t, name in enumerate(("nb_same", "nb_other", "nb_empty", "nb_out")):
        grains[name] = nb[:, t]
    grains["first_theta"], grains["first_phi"] = th, ph
    out["grains"] = grains
    return out


def write_grains_csv(path, grains):
    """The per-grain table of :func:`grain_metrics` (its "grains" entry) as a CSV with one row per grain."""
    import csv
    names = list(grains)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(names)
        for i in range(len(grains["id"])):
            w.writerow([grains[n][i].item() for n in names])


SOLID_COLUMNS = ("SolidVoxels", "Remelted", "G_solid", "Gi_solid", "Cool_solid", "T_solid", "V_solid", "G_over_V_solid")


def solid_metrics(profile, scales, remelted=0, step=0, clusters=None):
    """Columns of a metrics row (SOLID_COLUMNS) from one lattice's solidification profile (Engine.solid_profile, or entry r
    of Ensemble.solid_profile: dict(layers=..., grains=... or None)) taken with the quantisation ``scales``, plus the
    per-plane table under "planes" (rows of solid_layers.csv, tagged with ``step``) and, when the profile has grain records,
    the per-grain table under "grains" (rows of solid_grains.csv; ``clusters``, the row's clustering as Engine.clusters
    returns it, puts each grain's size n and bounding-box aspect beside its thermal history).

    SolidVoxels: voxels holding a record (solidified since the map began and not remelted; bad ones included).  Remelted:
    ``remelted``, the running count of cleared voxels.  G_solid, Gi_solid, Cool_solid, T_solid: means over the good records
    of |grad T| [K/m], its component along the build direction [K/m], the cooling rate [K/s] and the temperature [K] AT THE
    MOMENT EACH VOXEL SOLIDIFIED, from the quantised integer sums (sum / (n * scale)); 0.0 without a good record.
    V_solid = -Cool_solid / Gi_solid [m/s], the velocity of the isotherm the voxels froze on (0.0 when Gi_solid is 0);
    G_over_V_solid = G_solid / V_solid (inf for V_solid == 0)."""
    sc = [float(x) for x in scales]

    def means(rec):
        n = np.asarray(rec["n_rec"], dtype=np.int64).reshape(-1)
        q = np.asarray(rec["q"], dtype=np.int64).reshape(len(n), 4).astype(np.float64)
        safe = np.maximum(n, 1).astype(np.float64)
        return n, [np.where(n > 0, q[:, c] / (safe * sc[c]), 0.0) for c in range(4)]

    def table(rec, n, m):
        st_min = np.asarray(rec["stamp_min"], dtype=np.int64).reshape(-1)
        st_sum = np.asarray(rec["stamp_sum"], dtype=np.int64).reshape(-1)
        return {"n_rec": n, "n_bad": np.asarray(rec["n_bad"], dtype=np.int64).reshape(-1),
                "n_cooling": np.asarray(rec["n_cooling"], dtype=np.int64).reshape(-1),
                "G": m[0], "Gi": m[1], "Cool": m[2], "T": m[3],
                "stamp_first": np.where(n > 0, st_min, -1), "stamp_last": np.asarray(rec["stamp_max"], dtype=np.int64).reshape(-1),
                "stamp_mean": np.where(n > 0, st_sum / np.maximum(n, 1), -1.0)}

    lay = profile["layers"]
    n, m = means(lay)
    tot = int(n.sum())
    q_tot = np.asarray(lay["q"], dtype=np.int64).reshape(len(n), 4).sum(axis=0)
    G, Gi, cool, Ts = [(float(q_tot[c]) / (tot * sc[c]) if tot else 0.0) for c in range(4)]
    V = (-cool / Gi) if Gi != 0.0 else 0.0
    out = {"SolidVoxels": tot + int(np.asarray(lay["n_bad"], dtype=np.int64).sum()), "Remelted": int(remelted),
           "G_solid": G, "Gi_solid": Gi, "Cool_solid": cool, "T_solid": Ts, "V_solid": V,
           "G_over_V_solid": (G / V) if V != 0.0 else float("inf")}
    planes = {"Step": np.full(len(n), int(step), np.int64), "plane": np.arange(len(n), dtype=np.int64)}
    planes.update(table(lay, n, m))
    out["planes"] = planes
    if profile.get("grains") is not None:
        gr = profile["grains"]
        ng, mg = means(gr)
        grains = {"id": np.arange(1, len(ng) + 1, dtype=np.int64)}
        if clusters is not None:
            bb = np.asarray(clusters["bbox"], dtype=np.int64).reshape(-1, 6)
            d = bb[:, 3:] - bb[:, :3] + 1
            grains["n"] = np.asarray(clusters["size"], dtype=np.int64).reshape(-1)
            grains["aspect"] = (d.max(axis=1).astype(np.float64) / np.maximum(d.min(axis=1), 1).astype(np.float64)) if len(d) else np.zeros(0)
        grains.update(table(gr, ng, mg))
        out["grains"] = grains
    return out


def write_solid_csv(path, tables):
    """solid_layers.csv / solid_grains.csv: the tables of :func:`solid_metrics` ("planes": one per metrics row, written one
    below the other; "grains": the last row's) as a CSV."""
    import csv
    names = list(tables[0])
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(names)
        for t in tables:
            for i in range(len(t[names[0]])):
                w.writerow([t[n][i].item() for n in names])


ORIGIN_COLUMNS = ("Origin_dep", "Origin_nuc", "Origin_att", "Origin_hop", "Origin_unrecorded", "Nucleated_voxel_frac",
                  "Grains_born_nuc", "Grains_born_dep", "Grains_born_att", "Grains_born_hop", "Grains_substrate",
                  "Nucleated_grain_volume_frac", "Nuc_events", "Nuc_events_mean_i")
ORIGIN_CODE_NAMES = ("dep", "nuc", "att", "hop")      # fill codes 1..4 of an origin word


def origin_metrics(profile, census, step=0):
    """Columns of a metrics row (ORIGIN_COLUMNS) from one lattice's origin profile (Engine.origin_profile, or entry r of
    Ensemble.origin_profile: dict(layers=..., grains=... or None)) and its census (L, 5), plus the per-plane table under
    "planes" (rows of origin_layers.csv, tagged with ``step``) and, when the profile has grain records, the per-grain table
    under "grains" (rows of origin_grains.csv).

    Origin_dep / _nuc / _att / _hop: occupied voxels whose last recorded event was a deposition, a nucleation, an attachment
    to an existing grain, the arrival of a diffusing atom; Origin_unrecorded: occupied voxels without such a record
    (substrate, uploads).  Nucleated_voxel_frac: nuc over the four fill counts (0.0 when there are none).  A grain is born
    where its earliest recorded voxel was filled (the code inside ``birth``): Grains_born_nuc / _dep / _att / _hop count
    the grains all of whose voxels are recorded (n_unrec == 0) by that code, Grains_substrate those with n_unrec > 0.
    Nucleated_grain_volume_frac: the volume (n_occ) of the nucleation-born grains over all labelled volume -- the equiaxed
    fraction read from provenance instead of a bounding box (0.0 without grains).  Nuc_events: nucleation events absorbed
    since the map began, overwritten ones included; Nuc_events_mean_i: their mean build-plane index (0.0 when none)."""
    lay = profile["layers"]
    n_by = np.asarray(lay["n_by"], dtype=np.int64).reshape(-1, 4)
    by = n_by.sum(axis=0)
    filled = int(by.sum())
    cen = np.asarray(census, dtype=np.int64).reshape(-1, 5)
    nuc_ev = int(cen[:, 2].sum())
    out = {"Origin_dep": int(by[0]), "Origin_nuc": int(by[1]), "Origin_att": int(by[2]), "Origin_hop": int(by[3]),
           "Origin_unrecorded": int(np.asarray(lay["n_unrec"], dtype=np.int64).sum()),
           "Nucleated_voxel_frac": (float(by[1]) / filled) if filled else 0.0}
    born = {c: 0 for c in ORIGIN_CODE_NAMES}
    substrate, vol_nuc, vol_all = 0, 0, 0
    gr = profile.get("grains")
    if gr is not None:
        g_occ = np.asarray(gr["n_occ"], dtype=np.int64).reshape(-1)
        g_unrec = np.asarray(gr["n_unrec"], dtype=np.int64).reshape(-1)
        g_code = (np.asarray(gr["birth"], dtype=np.int64).reshape(-1) >> 24) & 7
        whole = g_unrec == 0
        for c, name in enumerate(ORIGIN_CODE_NAMES, start=1):
            born[name] = int(np.count_nonzero(whole & (g_occ > 0) & (g_code == c)))
        substrate = int(np.count_nonzero(g_unrec > 0))
        vol_all = int(g_occ.sum())
        vol_nuc = int(g_occ[whole & (g_occ > 0) & (g_code == 2)].sum())
    out.update({"Grains_born_nuc": born["nuc"], "Grains_born_dep": born["dep"], "Grains_born_att": born["att"],
                "Grains_born_hop": born["hop"], "Grains_substrate": substrate,
                "Nucleated_grain_volume_frac": (float(vol_nuc) / vol_all) if vol_all else 0.0,
                "Nuc_events": nuc_ev,
                "Nuc_events_mean_i": (float((cen[:, 2] * np.arange(len(cen), dtype=np.int64)).sum()) / nuc_ev) if nuc_ev else 0.0})

    def table(rec):
        n_occ = np.asarray(rec["n_occ"], dtype=np.int64).reshape(-1)
        nb = np.asarray(rec["n_by"], dtype=np.int64).reshape(-1, 4)
        nf = nb.sum(axis=1)
        birth = np.asarray(rec["birth"], dtype=np.int64).reshape(-1)
        t = {"n_occ": n_occ, "n_dep": nb[:, 0].copy(), "n_nuc": nb[:, 1].copy(), "n_att": nb[:, 2].copy(), "n_hop": nb[:, 3].copy(),
             "n_unrec": np.asarray(rec["n_unrec"], dtype=np.int64).reshape(-1),
             "n_left": np.asarray(rec["n_left"], dtype=np.int64).reshape(-1),
             "ord_first": np.where(nf > 0, np.asarray(rec["ord_min"], dtype=np.int64).reshape(-1), -1),
             "ord_last": np.asarray(rec["ord_max"], dtype=np.int64).reshape(-1),
             "ord_mean": np.where(nf > 0, np.asarray(rec["ord_sum"], dtype=np.int64).reshape(-1) / np.maximum(nf, 1), -1.0),
             "birth_code": np.where(nf > 0, (birth >> 24) & 7, 0), "birth_voxel": np.where(nf > 0, birth & ((1 << 24) - 1), -1)}
        return t

    planes = {"Step": np.full(len(n_by), int(step), np.int64), "plane": np.arange(len(n_by), dtype=np.int64)}
    planes.update(table(lay))
    planes.update({"ev_dep": cen[:, 0].copy(), "ev_diff_out": cen[:, 1].copy(), "ev_nuc": cen[:, 2].copy(), "ev_att": cen[:, 3].copy(),
                   "ev_diff_in": cen[:, 4].copy()})
    out["planes"] = planes
    if gr is not None:
        grains = {"id": np.arange(1, len(np.asarray(gr["n_occ"]).reshape(-1)) + 1, dtype=np.int64)}
        grains.update(table(gr))
        out["grains"] = grains
    return out


def write_origin_csv(path, tables):
    """origin_layers.csv / origin_grains.csv: the tables of :func:`origin_metrics` ("planes": one per metrics row, written
    one below the other; "grains": the last row's) as a CSV."""
    write_solid_csv(path, tables)


def front_velocity(row, prev, voxel_size=VOXEL_SIZE):
    """V_front of a metrics row: (Front_i - the previous row's) * voxel_size / (Time - the previous row's) in m/s; 0.0 on
    the first row (``prev`` None), when the time difference is 0 or when either row has no front."""
    if prev is None or not row["FrontVoxels"] or not prev.get("FrontVoxels"):
        return 0.0
    dt = float(row["Time"]) - float(prev["Time"])
    return (float(row["Front_i"]) - float(prev["Front_i"])) * voxel_size / dt if dt != 0.0 else 0.0


def compute_CET(state, theta, phi, voxel_size=VOXEL_SIZE):
    m = compute_metrics(state, theta, phi, voxel_size=voxel_size)
    ok = m["AspectRatio"] < CET_AR_THRESHOLD and m["EquiaxedFraction"] > CET_EQ_THRESHOLD
    return "Equiaxed" if ok else "Columnar"


def detect_CET_transition(metrics_dict):
    return (metrics_dict["AspectRatio"] < CET_AR_THRESHOLD and
            metrics_dict["EquiaxedFraction"] > CET_EQ_THRESHOLD)
