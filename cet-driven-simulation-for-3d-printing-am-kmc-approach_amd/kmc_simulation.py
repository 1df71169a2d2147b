"""Rejection-free KMC stepping loop on the GPU (drop-in for the reference ``kmc_simulation.py``).

``run_kmc`` keeps the reference's signature, return tuple, prints and ``metrics.csv`` contract
(kmc_simulation.py:203-398).  The hot loop -- thermal update every 20 steps, full-lattice rate
sweep, cumulative-rate event pick, lattice update -- runs on the device in batches through
``cetkmc_run_steps`` with NO host round trip per step; the host only

  * pre-draws the random streams from the very generators the reference uses (CPython
    ``random`` for the pick / defect / time draws, NumPy's legacy global stream for the
    deposition-species and orientation draws) and afterwards rewinds them to exactly the
    position the reference would have reached, and
  * runs the analysis that is not part of the hot path (defect-mask refresh and metrics every
    ``METRIC_UPDATE_STEP`` steps).

``run_kmc(mode="B", box=8)`` runs the same model through the synchronous super-step engine (``cetkmc_run_supersteps``:
thousands of events per rate sweep, NOT the reference's trajectory -- DESIGN.md "Mode B"), with the same prints and the same
18-column ``metrics.csv``.

There is no CPU fallback; without libcetkmc_hip.so + a GPU this raises.
"""
import os
import random

import numpy as np
import pandas as pd

from constants import (ATOMIC_SPACING_W, CET_CHECK_INTERVAL, DEFECT_ID, LATTICE_SIZE,  # noqa: F401
                       METRIC_UPDATE_STEP, N_STEPS, NU_DEP, RANDOM_SEED, RATE_THRESHOLD, T_MELT, T_SUB,
                       VOXEL_SIZE)
from defects import draw_defect_sites, introduce_defects, refresh_defects_device
from kmc_event_rates import get_event_rates  # noqa: F401  (re-exported like the reference)
from lattice_init import initialize_lattice
from metrics import (compute_CET, compute_metrics, compute_metrics_device, compute_metrics_from_clusters,  # noqa: F401
                     detect_CET_transition, front_metrics as _front_metrics, front_velocity as _front_velocity,
                     layer_metrics as _layer_metrics, texture_metrics as _texture_metrics,
                     write_layers_csv as _write_layers_csv, write_texture_csv as _write_texture_csv,
                     grain_metrics as _grain_metrics, write_grains_csv as _write_grains_csv,
                     solid_metrics as _solid_metrics, write_solid_csv as _write_solid_csv,
                     origin_metrics as _origin_metrics, write_origin_csv as _write_origin_csv)
from constants import CET_AR_THRESHOLD, CET_EQ_THRESHOLD
from thermal_solver import SCAN_PATTERNS, beam_table, laser_scan_planes, scan_path, stable_substeps
from thermal_solver import update_temperature_cet as update_temperature  # noqa: F401

# What the last run_kmc call observed besides its return tuple (the reference's signature has no room for it):
#   min_margin  smallest selection margin of the run (cetkmc_run_result.min_margin: distance of r = u * total from the nearer
#               end of the chosen event's interval of the cumulative rate sum, relative to the total).  The device sums rates by
#               a balanced tree, the reference left to right (kmc_simulation.py:259,265-274); the two sums differ by <= ~1e-13
#               relative, so only a pick with a margin below MARGIN_WARN could have gone to the neighbouring event there.
last_run_info = {}
MARGIN_WARN = 1e-12

THERMAL_EVERY = 20          # kmc_simulation.py:248
THERMAL_DT = 1e-6           # kmc_simulation.py:250
_MAX_STREAM_DOUBLES = 1 << 25   # host staging cap for the pre-drawn NumPy stream (256 MiB)


LASER_KEYS = ("power", "start", "speed", "beam_radius", "absorptivity", "latent")


BEAM_KEYS = ("power", "path", "beam_radius", "absorptivity", "latent", "depth", "penetration", "cutoff")
PATH_KEYS = ("pattern", "speed", "hatch", "start", "margin")


def _check_laser(laser, where="laser"):
    """A laser scan description.  Without ``path``: the plane route (thermal_solver.laser_scan_planes), dict with power, start,
    speed and optionally beam_radius, absorptivity, latent.  With ``path`` (dict with pattern, speed and optionally hatch, start,
    margin: thermal_solver.scan_path): the beam route, optionally depth, penetration, cutoff
    (thermal_solver.beam_table).  Returns a copy."""
    if isinstance(laser, dict) and "path" in laser:
        path = laser["path"]
        bad, missing = set(laser) - set(BEAM_KEYS), {"power", "path"} - set(laser)
        if bad or missing:
            raise ValueError(f"{where}: unknown keys {sorted(bad)}, missing keys {sorted(missing)} (allowed beside 'path': {', '.join(BEAM_KEYS)})")
        if not isinstance(path, dict) or set(path) - set(PATH_KEYS) or {"pattern", "speed"} - set(path):
            raise ValueError(f"{where}['path'] must be a dict with keys pattern, speed[, hatch, start, margin] (got {path!r})")
        if path["pattern"] not in SCAN_PATTERNS:
            raise ValueError(f"{where}['path']['pattern'] must be one of {SCAN_PATTERNS} (got {path['pattern']!r})")
        return dict(laser, path=dict(path))
    if not isinstance(laser, dict):
        raise ValueError(f"{where} must be a dict with keys power, start, speed[, beam_radius, absorptivity, latent]")
    bad, missing = set(laser) - set(LASER_KEYS), {"power", "start", "speed"} - set(laser)
    if bad or missing:
        raise ValueError(f"{where}: unknown keys {sorted(bad)}, missing keys {sorted(missing)} (allowed: {', '.join(LASER_KEYS)})")
    return dict(laser)


def beam_laser(power, pattern, speed, hatch=None, depth=1, penetration=None):
    """run_kmc's ``laser`` dict of the beam route, as the drivers' --scan / --hatch / --beam-depth / --penetration flags build it"""
    path = dict(pattern=pattern, speed=float(speed), **({"hatch": float(hatch)} if hatch is not None else {}))
    return dict(power=float(power), path=path, depth=int(depth), **({"penetration": float(penetration)} if penetration is not None else {}))


def _beam_table_of(laser, L, n_steps):
    """the beam table of a laser dict with a ``path`` for the updates of global steps [0, n_steps): ordinals 0 .. ceil(n / 20) - 1"""
    kw = {k: laser[k] for k in ("beam_radius", "absorptivity", "depth", "penetration", "cutoff") if k in laser}
    return beam_table(L, scan_path(L, **laser["path"]), 0, max(1, -(-int(n_steps) // THERMAL_EVERY)), laser["power"], **kw)


def _beam_table_of_layer(laser, L, layer, per_layer):
    """the beam table of build layer ``layer``: the global update ordinals layer * U .. (layer + 1) * U - 1,
    U = per_layer / 20, scan the path from its beginning again -- row u holds path(u - layer * U)"""
    kw = {k: laser[k] for k in ("beam_radius", "absorptivity", "depth", "penetration", "cutoff") if k in laser}
    U = int(per_layer) // THERMAL_EVERY
    path = scan_path(L, **laser["path"])
    return beam_table(L, lambda u: path(int(u) - layer * U), layer * U, max(1, U), laser["power"], **kw)


BUILD_KEYS = ("layers", "thickness", "T", "state")


def _check_build(build, L, n_steps, mode, checkpointing):
    """run_kmc's ``build`` (layer-by-layer builds): None, or a dict with layers, thickness and optionally T
    (temperature of a recoated layer, default T_SUB) and state (its state, default 0).  Returns a checked copy."""
    if build is None:
        return None
    if not isinstance(build, dict) or set(build) - set(BUILD_KEYS) or {"layers", "thickness"} - set(build):
        raise ValueError(f"build must be a dict with keys layers, thickness[, T, state] (got {build!r})")
    if mode != "A":
        raise ValueError("build needs mode 'A' (the layers are stepped by the exact loop)")
    if checkpointing:
        raise ValueError("build cannot be combined with checkpoint_every / resume_from (a checkpoint does not carry the layer state)")
    layers, h, state = int(build["layers"]), int(build["thickness"]), int(build.get("state", 0))
    if layers < 1:
        raise ValueError(f"build: layers must be >= 1 (got {build['layers']!r})")
    if not 1 <= h <= L - 1:
        raise ValueError(f"build: thickness must lie in 1 .. L - 1 = {L - 1} (got {build['thickness']!r})")
    if not 0 <= state <= 4:
        raise ValueError(f"build: state must lie in 0 .. 4 (got {build['state']!r})")
    if int(n_steps) <= 0 or int(n_steps) % THERMAL_EVERY:
        raise ValueError(f"build: n_steps is the number of steps per layer and must be a positive multiple of {THERMAL_EVERY}, so that "
                         f"every layer begins on a temperature-update step (got {n_steps})")
    return dict(layers=layers, thickness=h, T=float(build.get("T", T_SUB)), state=state)


def _retired_planes(tables, count, layer, height0):
    """rows of build_layers.csv: planes 0 .. count - 1 of a metrics row's per-plane tables (``tables``: name -> the
    "planes" dict of metrics.layer_metrics / solid_metrics / origin_metrics), tagged with the layer that retires them and their
    height in the finished part, ``height0`` + the plane index"""
    rows = []
    for p in range(count):
        row = {"Layer": int(layer), "BuildHeight": int(height0 + p), "Plane": int(p)}
        for name, t in tables.items():
            for col, values in t.items():
                if col != "plane":
                    row[f"{name}_{col}"] = values[p].item()
        rows.append(row)
    return rows


def _check_beam_route(laser, scheme, L):
    """a laser with a path needs the implicit scheme (the explicit kernels read a source plane), and a path and a depth profile
    that thermal_solver accepts for this L (checked on a one-row table, before any device call)"""
    if laser is None or "path" not in laser:
        return
    if scheme != "implicit":
        raise ValueError("a laser with a 'path' takes the beam route, which needs thermal_scheme='implicit'")
    _beam_table_of(laser, L, 1)


def _draw_uniforms(per, n, per_step):
    """The host streams of n steps from the global generators: ``per`` CPython uniforms per step (pick[, defect], time) and
    ``per_step`` NumPy uniforms per step.  Returns (generator states before the draws, draws[n, per], u_np)."""
    py_state = random.getstate()
    draws = np.array([random.random() for _ in range(per * n)], dtype=np.float64).reshape(n, per)
    np_state = np.random.get_state()
    return (py_state, np_state), draws, np.random.random(n * per_step)


def _rewind_uniforms(saved, per, n, done, np_used):
    """Both global generators back to what the ``done`` executed steps of ``n`` consumed (``np_used`` NumPy uniforms)."""
    py_state, np_state = saved
    np.random.set_state(np_state)
    if np_used:
        np.random.random(np_used)
    if done < n:
        random.setstate(py_state)
        for _ in range(per * done):
            random.random()


def _nominal_gr(L, nu_dep):
    """Nominal (G, R, R_phys, G_over_R_phys) of a run: kmc_simulation.py:229-232."""
    G = (T_MELT - T_SUB) / (L * VOXEL_SIZE)
    R_phys = nu_dep * ATOMIC_SPACING_W
    return G, nu_dep * 2.74e-10 / VOXEL_SIZE, R_phys, G / R_phys


def _write_metrics(output_prefix, rows):
    """outputs/<prefix>/metrics.csv, and metrics_<tag>.csv beside it: plot_cet.py globs outputs/impurity_c_*/metrics_*.csv
    (plot_cet.py:26).  Returns the first path."""
    df = pd.DataFrame(rows)
    output_path = os.path.join(f"outputs/{output_prefix}", "metrics.csv")
    df.to_csv(output_path, index=False)
    df.to_csv(os.path.join(f"outputs/{output_prefix}", f"metrics_{output_prefix.split('_')[-1]}.csv"), index=False)
    return output_path


def _advance_to(engine, first, last, L, defect_fraction, rng_mode=0, seed=0, incremental=True, thermal_mode=1, laser=None):
    """Run steps first..last (inclusive) on the device.  Returns (steps_done, terminated,
    last_total, dt_sum_increments, min_margin) with both host generators left where the reference's would be.
    ``laser``: the temperature updates are thermal_mode 2 with the scan's source planes of each batch (a plane depends on
    the global step only, so a batch continued from a status-2 stop is handed the plane of its first step again)."""
    dts = []
    min_margin = 1.0
    step = first
    terminated = False
    last_total = 0.0
    per = 3 if defect_fraction > 0.0 else 2
    slack = 8
    while step <= last:
        n = last - step + 1
        if rng_mode == 0:
            # One deposition-species draw per finite-rate deposition candidate per step (kmc_event_rates.py:63-65) + 2
            # orientation draws.  The candidate count is asked from the device (one sweep) instead of assuming the
            # whole top plane (L*L): at L = 256 that assumption means ~13 M doubles drawn, uploaded and re-drawn per
            # 200-step batch.  A batch that still runs short stops with status 2 and is continued from there.
            n_dep_now = int(engine.rate_sweep()[2])
            per_step = min(L * L, n_dep_now + slack) + 2
        else:
            per_step = 2
        n = max(1, min(n, _MAX_STREAM_DOUBLES // per_step))
        saved, draws, u_np = _draw_uniforms(per, n, per_step)
        q = laser_scan_planes(L, laser, step, n) if laser is not None and "path" not in laser else None       # (a path: the handle's beam table)
        res = engine.run_steps(step, n, defect_fraction, draws[:, 0], draws[:, 1] if per == 3 else None, u_np,
                               rng_mode=rng_mode, seed=seed, thermal_mode=2 if laser is not None else thermal_mode,
                               thermal_dt=THERMAL_DT, incremental=incremental, q_planes=q if q is not None and len(q) else None,
                               use_latent=bool(laser.get("latent", True)) if laser is not None else True)
        done = res["done"]
        min_margin = min(min_margin, res["min_margin"])
        _rewind_uniforms(saved, per, n, done, res["np_used"])
        for s in range(done):
            total = res["totals"][s]
            dts.append(max(-np.log(max(1e-12, draws[s, per - 1])) / total, 1e-12))   # kmc_simulation.py:331
        step += done
        if res["status"] == 1:
            terminated = True
            last_total = float(res["totals"][done]) if len(res["totals"]) > done else 0.0
            break
        if res["status"] == 2 and done == 0:
            if slack >= L * L:
                raise RuntimeError("pre-drawn NumPy stream too small for a single step")
            slack = min(L * L, 4 * slack + 64)       # the estimate was short (candidates appeared): widen and retry
    return step - first, terminated, last_total, dts, min_margin


def _metrics_row(cl, counts, nuc, L, step, total_time, n_flagged, nuc_offset, cet_detected, G, R, R_phys, G_over_R_phys):
    """One metrics.csv row (kmc_simulation.py:339-389) of a lattice after event index ``step`` from its clustering ``cl``,
    species ``counts`` and nucleation count ``nuc`` (computed on the device)."""
    m = compute_metrics_from_clusters(cl, L ** 3, defects_count=n_flagged, voxel_size=VOXEL_SIZE)
    defect_voxels = int(counts[DEFECT_ID])
    m["Defect_voxel_count"] = defect_voxels
    m["DefectDensity"] = float(defect_voxels / (L ** 3))
    if (not cet_detected) and detect_CET_transition(m):
        cet_detected = True
        print(f"CET detected at step {step} (G/R={G / R:.2e})")
    return {
        "Step": step,
        "Time": total_time,
        "AspectRatio": m["AspectRatio"],
        "EquiaxedFraction": m["EquiaxedFraction"],
        "NucleationDensity": m["NucleationDensity"],
        "DefectDensity": m["DefectDensity"],
        "AvgGrainSize": m["AvgGrainSize"],
        "GrainCount": m["GrainCount"],
        "W_Count": int(counts[1]),
        "Re_Count": int(counts[2]),
        "C_Count": int(counts[3]),
        "NucleationCount": nuc_offset + nuc,
        "G_over_R": (G / R) if R > 0 else np.inf,
        "G_phys": G,
        "R_phys": R_phys,
        "G_over_R_phys": G_over_R_phys,
        # compute_CET re-clusters the same lattice (metrics.py:99-101): same AR / equiaxed fraction
        "CET_Class": "Equiaxed" if (m["AspectRatio"] < CET_AR_THRESHOLD and m["EquiaxedFraction"] > CET_EQ_THRESHOLD) else "Columnar",
        "CET_Detected": cet_detected,
    }


def _add_front_columns(row, stats, L, prev):
    """front_metrics=True: the measured front columns (metrics.front_metrics) and V_front behind the 18 columns of ``row``;
    ``prev`` is the run's previous row (None on the first)."""
    row.update(_front_metrics(stats, L, VOXEL_SIZE))
    row["V_front"] = _front_velocity(row, prev, VOXEL_SIZE)
    return row


def _add_layer_columns(row, profile, L):
    """layer_metrics=True: the layer columns (metrics.LAYER_COLUMNS) behind every other column of ``row``, in place;
    returns the per-plane table of the row (the rows of layers.csv)."""
    m = _layer_metrics(profile, L, VOXEL_SIZE)
    planes = m.pop("planes")
    row.update(m)
    return planes


def _add_texture_columns(row, profile):
    """texture_metrics=True: the texture columns (metrics.TEXTURE_COLUMNS) behind every other column of ``row``, in place;
    returns the per-plane table of the row (the rows of texture.csv)."""
    m = _texture_metrics(profile)
    planes = m.pop("planes")
    row.update(m)
    return planes


def _add_grain_columns(row, table):
    """grain_metrics=True: the grain columns (metrics.GRAIN_COLUMNS) behind every other column of ``row``, in place; returns
    the per-grain table of the row (the rows of grains.csv)."""
    m = _grain_metrics(table, VOXEL_SIZE)
    grains = m.pop("grains")
    row.update(m)
    return grains


def _add_solid_columns(row, profile, scales, remelted, clusters):
    """solid_metrics=True: the solidification columns (metrics.SOLID_COLUMNS) behind every other column of ``row``, in place;
    returns the per-plane table of the row (rows of solid_layers.csv) and the per-grain one (solid_grains.csv) or None."""
    m = _solid_metrics(profile, scales, remelted, row["Step"], clusters)
    planes, grains = m.pop("planes"), m.pop("grains", None)
    row.update(m)
    return planes, grains


def _add_origin_columns(row, profile, census):
    """origin_metrics=True: the origin columns (metrics.ORIGIN_COLUMNS) behind every other column of ``row``, in place;
    returns the per-plane table of the row (rows of origin_layers.csv) and the per-grain one (origin_grains.csv) or None."""
    m = _origin_metrics(profile, census, row["Step"])
    planes, grains = m.pop("planes"), m.pop("grains", None)
    row.update(m)
    return planes, grains


def _remelt_threshold(remelt, where="remelt"):
    """run_kmc's ``remelt`` option as a threshold temperature: None for off (False / None), T_MELT for True, else the number"""
    if remelt is None or remelt is False:
        return None
    if remelt is True:
        return float(T_MELT)
    if isinstance(remelt, (int, float, np.integer, np.floating)) and not np.isnan(float(remelt)):
        return float(remelt)
    raise ValueError(f"{where} must be False, True (melt at T_MELT) or a threshold temperature")


def _thermal_substeps(value, where="thermal_substeps"):
    """run_kmc's ``thermal_substeps`` option as a count: an integer >= 1, or "stable" = thermal_solver.stable_substeps(1e-6)"""
    if isinstance(value, str) and value == "stable":
        return stable_substeps(THERMAL_DT)
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < 1:
        raise ValueError(f"{where} must be an integer >= 1 or 'stable' (got {value!r})")
    return int(value)


def _apply_thermal_options(target, n_sub, scheme, boundary, remelt_thr):
    """the four thermal options of run_kmc / run_kmc_ensemble on their Engine / Ensemble; a default stays unset"""
    if remelt_thr is not None:
        target.set_remelt(True, remelt_thr)
    if n_sub != 1:
        target.set_thermal_substeps(n_sub)
    if scheme != "explicit":
        target.set_thermal_scheme(scheme)
    if boundary is not None:
        target.set_thermal_boundary(boundary)


def _check_substeps(n_sub, mode_a, thermal_updates):
    """what run_kmc and run_kmc_ensemble refuse of thermal_substeps > 1 (before any device call)"""
    if n_sub == 1:
        return
    if not mode_a:
        raise ValueError("thermal_substeps needs mode 'A' (the super-step engine's updates are not sub-stepped)")
    if not thermal_updates:
        raise ValueError("thermal_substeps needs thermal_updates=True (there is no update to split)")


def _check_scheme(scheme, mode_a, thermal_updates, where="thermal_scheme", needs="mode 'A' (the super-step engine's updates are explicit)"):
    """what run_kmc and run_kmc_ensemble refuse of thermal_scheme (before any device call); ``needs``: what ``mode_a`` stands
    for in the caller's terms"""
    if scheme not in ("explicit", "implicit"):
        raise ValueError(f"{where} must be 'explicit' or 'implicit' (got {scheme!r})")
    if scheme == "explicit":
        return
    if not mode_a:
        raise ValueError(f"thermal_scheme='implicit' needs {needs}")
    if not thermal_updates:
        raise ValueError("thermal_scheme='implicit' needs thermal_updates=True (there is no update to make implicit)")


def run_gradient_boundary(L, temp=T_SUB, cooling_rate=0.0):
    """The boundary that holds the field a run starts from: ``initialize_lattice`` ramps T along axis 2 with the slope
    (T_MELT - temp) / L, so the two k faces are fixed at the ramp's next values, T(-1) and T(L); every other face adiabatic.
    (thermal_solver.gradient_boundary does the same for ``build_temperature_field``'s ramp along axis 0.)"""
    slope = (T_MELT - float(temp)) / L
    return dict(beta=[0.0, 0.0, 0.0, 0.0, 1.0, 1.0], T_ext=[0.0, 0.0, 0.0, 0.0, float(temp) - slope, float(temp) + slope * L],
                ramp=[0.0] * 4 + [-float(cooling_rate) * THERMAL_DT] * 2)


def _thermal_boundary(value, L, temp, mode_a, scheme, thermal_updates, needs="mode 'A' (the super-step engine's updates are explicit)"):
    """run_kmc's and run_kmc_ensemble's ``thermal_boundary`` option as dict(beta, T_ext, ramp) of six floats each, or None;
    what they refuse of it (before any device call)"""
    if value is None:
        return None
    if not mode_a:
        raise ValueError(f"thermal_boundary needs {needs}")
    if scheme != "implicit":
        raise ValueError("thermal_boundary needs thermal_scheme='implicit' (the explicit update is adiabatic)")
    if not thermal_updates:
        raise ValueError("thermal_boundary needs thermal_updates=True (there is no update to bound)")
    if isinstance(value, str) and value == "gradient":
        return run_gradient_boundary(L, temp)
    try:
        out = {k: [float(x) for x in value.get(k, [0.0] * 6)] if k != "beta" else [float(x) for x in value["beta"]] for k in ("beta", "T_ext", "ramp")}
        if all(len(v) == 6 for v in out.values()):
            return out
    except (AttributeError, KeyError, TypeError, ValueError):
        pass
    raise ValueError(f"thermal_boundary must be None, 'gradient' or a dict of six beta, T_ext and ramp values "
                     f"(thermal_solver.thermal_boundary); got {value!r}")


def _check_remelt(thr, mode_a, origin_metrics, thermal_updates):
    if thr is None:
        return
    if not mode_a:
        raise ValueError("remelt needs mode 'A' (the super-step engine has no melt)")
    if origin_metrics:
        raise ValueError("remelt cannot be combined with origin_metrics (the event log the origin map folds holds no melts)")
    if not thermal_updates:
        raise ValueError("remelt needs thermal_updates=True (the melt follows the temperature update)")


def _add_remelt_columns(row, info, offset=(0, 0)):
    """remelt: the running totals of cetkmc_remelt_info behind every other column of ``row``, in place"""
    row["RemeltPasses"] = int(offset[0] + info["passes"])
    row["RemeltedVoxels"] = int(offset[1] + info["n_melted"])


def _check_origin(origin_metrics, checkpointing):
    if origin_metrics and checkpointing:
        raise ValueError("origin_metrics cannot be combined with checkpoint_every / resume_from (a checkpoint does not carry the map)")


def _check_solid(solid_metrics, solid_every, checkpointing):
    if not solid_metrics:
        return
    if isinstance(solid_every, bool) or not isinstance(solid_every, (int, np.integer)) or solid_every < THERMAL_EVERY or solid_every % THERMAL_EVERY:
        raise ValueError(f"solid_every must be a positive multiple of {THERMAL_EVERY} (the map is updated right before a temperature update)")
    if checkpointing:
        raise ValueError("solid_metrics cannot be combined with checkpoint_every / resume_from (a checkpoint does not carry the map)")


def _updates_between(a, b):
    """temperature updates issued at the global steps (or super-steps) a <= g < b: the multiples of THERMAL_EVERY there"""
    up = lambda x: -(-x // THERMAL_EVERY)        # noqa: E731
    return up(b) - up(a) if b > a else 0


def _print_row(step, row):
    print(
        f"Step {step}: AR={row['AspectRatio']:.2f}, "
        f"EqFrac={row['EquiaxedFraction']:.2f}, "
        f"NucDens={row['NucleationDensity']:.3e}, "
        f"DefectDens={row['DefectDensity']:.3e}, "
        f"CET={row['CET_Class']}, "
        f"Detected={row['CET_Detected']}, "
        f"Time={row['Time']:.2e}s"
    )


def save_checkpoint(path, fields, defects_mask, next_step, total_time, nucleation_count, metrics_data, cet_detected, extra=None):
    """Everything needed to continue a run bit-identically: the five lattice fields, the defect mask,
    the loop counters, the metrics rows so far and the state of BOTH host generators (CPython
    ``random`` and NumPy's legacy global stream).  The reference has no resume."""
    import json
    py = random.getstate()
    npst = np.random.get_state()
    tmp = path + ".tmp.npz"        # written beside the target and renamed into place: a crash mid-write keeps the old file
    np.savez_compressed(
        tmp, state=fields["state"].astype(np.int8), theta=fields["theta"], phi=fields["phi"], T=fields["T"],
        defects=np.asarray(defects_mask).astype(np.int8), next_step=next_step, total_time=total_time,
        nucleation_count=nucleation_count, cet_detected=bool(cet_detected),
        py_version=py[0], py_mt=np.array(py[1], dtype=np.uint64), py_gauss=np.array([np.nan if py[2] is None else py[2]]),
        np_mt=npst[1], np_pos=npst[2], np_has_gauss=npst[3], np_cached=npst[4],
        metrics_json=np.array(json.dumps(metrics_data, default=lambda o: o.item() if hasattr(o, "item") else str(o))),
        extra_json=np.array(json.dumps(extra or {})))          # mode "B": super-step index, temperature updates applied, seed, box
    os.replace(tmp, path)


def load_checkpoint(path):
    """Inverse of save_checkpoint; also restores both host generators."""
    import json
    z = np.load(path, allow_pickle=False)
    g = float(z["py_gauss"][0])
    random.setstate((int(z["py_version"]), tuple(int(x) for x in z["py_mt"]), None if np.isnan(g) else g))
    np.random.set_state(("MT19937", z["np_mt"], int(z["np_pos"]), int(z["np_has_gauss"]), float(z["np_cached"])))
    return dict(state=z["state"].astype(np.int64), theta=z["theta"], phi=z["phi"], T=z["T"],
                defects=z["defects"].astype(np.int64), next_step=int(z["next_step"]), total_time=float(z["total_time"]),
                nucleation_count=int(z["nucleation_count"]), cet_detected=bool(z["cet_detected"]),
                metrics_data=json.loads(str(z["metrics_json"])),
                extra=json.loads(str(z["extra_json"])) if "extra_json" in z.files else {})


def run_kmc(
    L: int = LATTICE_SIZE,
    n_steps: int = N_STEPS,
    temp: float = T_SUB,
    defect_fraction: float = 0.0,
    n_seeds: int = 5,
    impurity_c: float = 0.0,
    output_prefix: str = "cet_run",
    *,
    checkpoint_every: int = 0,
    resume_from: str = None,
    incremental: bool = True,
    nu_dep: float = None,
    mode: str = "A",
    box: int = 8,
    null_events: bool = True,
    thermal_cadence: str = "events",
    seed: int = None,
    metrics_every: int = METRIC_UPDATE_STEP,
    thermal_updates: bool = True,
    laser: dict = None,
    front_metrics: bool = False,
    layer_metrics: bool = False,
    texture_metrics: bool = False,
    grain_metrics: bool = False,
    solid_metrics: bool = False,
    solid_every: int = 20,
    origin_metrics: bool = False,
    remelt=False,
    thermal_substeps=1,
    thermal_scheme="explicit",
    thermal_boundary=None,
    local_events: int = 0,
    local_horizon: float = 1.0,
    build: dict = None,
):
    """KMC microstructure evolution with natural defect injection (same contract as the
    reference).  ``defect_fraction`` is the per-event probability that the just-updated voxel
    becomes a defect.

    Extensions (keyword-only, not in the reference): ``checkpoint_every=k`` writes
    ``outputs/<prefix>/checkpoint.npz`` every k steps (mode "B": after the super-step that reaches each multiple of k
    executed events); ``resume_from=path`` continues such a run --
    the continued run is bit-identical to an uninterrupted one (lattice, time, CSV, RNG streams), in both modes;
    ``incremental=False`` re-evaluates the whole lattice on every step like get_event_rates does (the
    default re-evaluates only the rows an event made stale between temperature updates -- same results);
    ``nu_dep`` overrides constants.NU_DEP (deposition attempt frequency = growth velocity V of the G-V sweep
    driver gv_sweep.py; the reference can only change it by editing constants.py);
    ``seed`` replaces constants.RANDOM_SEED for both host generators (and keys Mode B's counter uniforms);
    ``metrics_every`` replaces constants.METRIC_UPDATE_STEP (cadence of the metrics rows and of the defect-mask refresh);
    ``thermal_updates=False`` keeps the initial temperature field (no update_temperature_cet calls: a stationary
    environment, used to compare the two stepping modes without the reference's event-count thermal clock).

    ``mode="B"``: synchronous super-steps over ``(L/box)**3`` boxes (cetkmc_run_supersteps; ``box == L`` is the
    single-domain case = the exact loop with counter uniforms).  ``n_steps`` keeps its meaning -- the number of EXECUTED
    events -- and the run ends with the first super-step that reaches it (it may overshoot by less than one super-step;
    the last row's ``Step`` says by how much).  ``Step`` of a row = index of the last executed event, rows are written by
    the first super-step that reaches each multiple of ``metrics_every`` (and by the last one), ``Time`` advances per
    executed event as kmc_simulation.py:331-332 does.  ``null_events`` (default on): boxes execute with probability
    R_box / R_max, which makes every event's frequency proportional to its rate as in the reference's global pick.
    ``thermal_cadence="events"`` (default) keeps the reference's cadence of one temperature update per 20 executed events
    (kmc_simulation.py:248-250): before every super-step the field is brought to ``executed // 20 + 1`` updates;
    ``"supersteps"`` updates once per 20 super-steps inside the engine (throughput setting for large lattices: the
    temperature history per executed event then differs from the reference's).
    ``local_events=K > 0`` (mode "B", ``box`` 8) selects the local event loop (cetkmc_run_supersteps_local, DESIGN.md
    section 23): every box executes up to K events per super-step, until its waiting times pass the horizon
    ``local_horizon / R_max``; the event mix stays rate-proportional and ``null_events`` is not consulted.  Both
    ``thermal_cadence`` settings work, ``Time`` advances per executed event as above, and ``last_run_info`` gains
    ``horizon_time`` (the sum of horizon / 8 over the super-steps: the sublattice picture's clock) and ``capped_boxes``
    (boxes that stopped at K events).  With ``origin_metrics=True`` all events of a super-step share one ordinal of the
    origin map, whose fold keeps the largest (ordinal, code) word per voxel: a voxel that is left and filled again within
    ONE super-step (a hop away and another atom in) keeps the code "left" while occupied, and the origin columns count it
    as unrecorded.

    ``laser`` (mode "A"): every temperature update is the laser update of thermal_solver.update_temperature -- a moving
    Gaussian source on plane L-1 and, with ``latent`` (default on), latent heat where a voxel solidified since the previous
    update -- instead of update_temperature_cet.  A dict ``power``, ``start`` (beam centre at update 0, voxels), ``speed``
    (voxels per update) and optionally ``beam_radius``, ``absorptivity``, ``latent`` (thermal_solver.laser_scan_planes).
    prev_state lives on the device: the initial upload snapshots it and every update brings it level with state.
    A laser dict with a ``path`` (dict with pattern, speed and optionally hatch, start, margin: thermal_solver.scan_path) instead of
    ``start`` / ``speed`` takes the beam route: the scan follows the path ("diagonal", "line", "raster",
    "serpentine"), ``depth`` planes absorb the beam (``penetration`` [m]: e-folding depth; None: uniform), factors beyond
    ``cutoff`` radii are zero, and the device builds every update's source from one beam table copied once
    (cetkmc_set_beam); no plane crosses to the device.  It needs ``thermal_scheme="implicit"`` (ValueError otherwise) and composes
    with ``remelt``, ``thermal_substeps``, ``thermal_boundary`` and the diagnostics; ``last_run_info["beam"]`` reports the path,
    the depth and cetkmc_get_beam_info's totals.  A dict without ``path`` is the plane route, as before.
    Refused with ValueError: ``laser`` with ``mode="B"``; with ``checkpoint_every`` / ``resume_from`` (a checkpoint does not
    carry prev_state); with ``thermal_updates=False``.

    ``front_metrics=True`` (both modes, with and without ``laser``): every metrics row gains, behind its 18 columns, the
    measured front columns of metrics.front_metrics -- temperature gradient at the growth front, front position, melt-pool
    size, reduced on the device by cetkmc_front_stats (112 bytes cross PCIe per row) -- and ``V_front`` = (Front_i - the
    previous row's) * VOXEL_SIZE / (Time - the previous row's) in m/s (0.0 on the first row, for a zero time difference or
    when either row has no front; a resumed run takes the previous row from the checkpoint's rows).

    ``layer_metrics=True`` (both modes, with and without ``laser``): every metrics row gains, behind its 18 columns (and
    behind the front columns), the layer columns of metrics.layer_metrics -- the CET height, the equiaxed area fraction,
    the mean intercept lengths along and across the build direction and the species-resolved grain-boundary fractions --
    from the row's own clustering, reduced on the device by cetkmc_layer_profile (L * 144 bytes cross PCIe per row); the
    per-plane table of the last row is written to ``outputs/<prefix>/layers.csv``.

    ``texture_metrics=True`` (both modes, with and without ``laser``): every metrics row gains, behind the layer columns,
    the texture columns of metrics.texture_metrics -- grain-grain faces, their mean misorientation, the low-angle and
    lateral shares and the share of voxels aligned with the build axis -- from the row's own clustering, binned on the
    device by cetkmc_texture_profile (Engine.texture_profile's defaults: 36 bins, axis (1, 0, 0); L * 148 * 8 bytes cross
    PCIe per row); the per-plane table of the last row is written to ``outputs/<prefix>/texture.csv``.

    ``grain_metrics=True`` (both modes, with and without ``laser``): every metrics row gains, behind every other column, the
    grain columns of metrics.grain_metrics -- moment-based elongation and inclination of the grains, the columnar volume
    fraction, the largest grain's share, the same-grain share of the stencil contacts and the aligned volume fraction --
    from the row's own clustering, reduced on the device by cetkmc_grain_table (160 bytes per grain cross PCIe per row); the
    per-grain table of the last row is written to ``outputs/<prefix>/grains.csv``.

    ``solid_metrics=True`` (both modes, with and without ``laser``): the device keeps a solidification map (cetkmc_solid_*,
    DESIGN.md section 21) -- per voxel the step count, temperature, temperature gradient and cooling rate at the moment it
    solidified.  The map begins after the initial upload (the initial lattice is substrate); ``solid_every`` is a multiple
    of 20; dt = max(1, temperature updates since the previous map update) * 1e-6 s.  Mode A: the stepping batches are split
    at the multiples of ``solid_every`` and the map is updated there, right BEFORE the step whose temperature update is due:
    the recorded T is the field the batch's events saw and stamp = that multiple, the global step count.  Mode B: the map is
    updated AFTER the super-step batch in which the count of executed events reaches or passes a multiple of ``solid_every``;
    stamp = the events executed by then, which can lie up to (events per super-step - 1) past the multiple, and the recorded
    T is the field as that batch left it.  With ``thermal_cadence="events"`` that is the field its events saw; with the
    super-step cadence the engine updates T by the super-step index, not by the event count, so the field may already carry
    an update that followed the events.  A voxel that solidifies and empties again between
    two updates is not seen, and a row shows the map as of the last update (at most ``solid_every`` steps back).  Every
    metrics row gains, behind every other column, the columns of metrics.solid_metrics (per-lattice means at freezing,
    V_solid = -Cool_solid / Gi_solid, G_over_V_solid), reduced on the device by cetkmc_solid_profile under
    cetkmc.engine.default_solid_scales(); ``outputs/<prefix>/solid_layers.csv`` gets one row per plane and metrics row and,
    with ``grain_metrics=True``, ``solid_grains.csv`` one row per grain of the last row (thermal history beside the grain's
    size and bounding-box aspect).  Refused with ValueError: ``solid_every`` not a positive multiple of 20; together with
    ``checkpoint_every`` / ``resume_from`` (a checkpoint does not carry the map).

    ``origin_metrics=True`` (both modes, with and without ``laser``): the device keeps an origin map (cetkmc_origin_*,
    DESIGN.md section 22) -- per voxel how it was last filled (deposition, nucleation, attachment to an existing grain, a
    diffusion hop) and at which executed step (Mode A) or super-step (Mode B), folded on the device from the event log every
    stepping call writes there anyway; the stepping itself is unchanged.  The map begins after the initial upload (the
    initial lattice is unrecorded substrate).  Every metrics row gains, behind every other column, the columns of
    metrics.origin_metrics (voxels by origin, grains by the origin of their earliest voxel, the volume fraction of the
    nucleation-born grains, the nucleation events and their mean height), reduced on the device by cetkmc_origin_profile;
    ``outputs/<prefix>/origin_layers.csv`` gets one row per plane and metrics row and, with ``grain_metrics=True``,
    ``origin_grains.csv`` one row per grain of the last row (the grain records themselves always come from the row's own
    clustering).  Refused with ValueError together with ``checkpoint_every`` /
    ``resume_from`` (a checkpoint does not carry the map).

    ``remelt=True`` (or a threshold temperature; mode "A" only, with or without ``laser``): remelting on the device
    (cetkmc_set_remelt) -- behind every temperature update the occupied voxels with T >= T_MELT (or
    the given threshold) become empty, before that step's rates are evaluated.  Every metrics row gains, behind every other
    column, ``RemeltPasses`` and ``RemeltedVoxels`` (running totals); ``last_run_info["remelted"]`` carries the total.
    Checkpoints carry the setting and the totals (only then), and a resumed run must ask for the same threshold.  Refused
    with ValueError: ``mode="B"``, ``origin_metrics``, ``thermal_updates=False``.

    ``thermal_substeps=n`` (or ``"stable"`` = thermal_solver.stable_substeps(1e-6) = 17; mode "A" only, with or without
    ``laser`` and ``remelt``): every temperature update is n explicit steps of 1e-6 / n s on the device
    (cetkmc_set_thermal_substeps) -- the reference's single step is 16 times too long for the
    explicit scheme and turns a rough field into noise between the clip values.  ``last_run_info["thermal_substeps"]``
    reports n.  Checkpoints carry the value only when it is not 1, and a resumed run must ask for the same.  Refused with
    ValueError: ``mode="B"``, ``thermal_updates=False``.

    ``thermal_scheme="implicit"`` (mode "A" only, with or without ``laser``, ``remelt`` and ``thermal_substeps``): every
    temperature update is ``thermal_substeps`` locally one-dimensional backward-Euler steps on the device
    (cetkmc_set_thermal_scheme), stable at any dt.  ``last_run_info["thermal_scheme"]`` reports it.
    Checkpoints carry the value only when it is not "explicit", and a resumed run must ask for the same.  Refused with
    ValueError: ``mode="B"``, ``thermal_updates=False``.

    ``thermal_boundary`` (mode "A" with ``thermal_scheme="implicit"`` only): ``"gradient"`` holds the imposed gradient -- the two
    faces across the initial ramp are fixed at the ramp's next values (``run_gradient_boundary``), so the ramp is a fixed point
    of the update -- or a dict from ``thermal_solver.thermal_boundary`` (a substrate sink, convective faces, a cooling rate);
    cetkmc_set_thermal_boundary, DESIGN.md section 27.  ``last_run_info["thermal_boundary"]`` reports the dict (None without).
    Checkpoints carry it (``extra["thermal_bc"]``) only when it is set, and a resumed run must ask for the same.  Refused with
    ValueError: ``mode="B"``, any other ``thermal_scheme``, ``thermal_updates=False``.

    ``build=dict(layers=N, thickness=h, T=T_layer, state=0)`` (mode "A" only, with or without ``laser``): a layer-by-layer
    build.  ``n_steps`` becomes the number of steps PER LAYER, a positive multiple of 20, and the global
    step index runs on across the layers.  Behind the last metrics row of every layer but the last, the part is lowered by
    ``h`` planes on the device -- ``Engine.shift((-h, 0, 0), fill_state=state, fill_T=T)``: the bottom h planes leave, h planes
    of state ``state`` (default 0) at temperature ``T`` (default T_SUB) appear on top, the maps move along.  With
    ``layer_metrics``, ``solid_metrics`` or ``origin_metrics`` the per-plane records of the planes about to leave are appended
    to ``outputs/<prefix>/build_layers.csv`` with ``Layer`` and ``BuildHeight`` (plane index + h * the layers retired before),
    and at the end the remaining L planes: the file holds the whole part, L + (N - 1) h planes.  A laser with a ``path`` scans
    the path from its beginning in every layer (a fresh beam table per layer); the plane route goes on unchanged.  Every
    metrics row gains ``Layer`` behind every other column; ``last_run_info["build"]`` carries layers, thickness, the retired
    planes, the voxels that left, by species, and ``complete`` (False when the run terminated early: build_layers.csv then ends with the
    retired planes).  Refused with ValueError: ``mode="B"``; ``checkpoint_every`` / ``resume_from``
    (a checkpoint does not carry the layer state); ``thickness`` outside 1 .. L - 1; ``layers`` < 1; ``n_steps`` not a
    positive multiple of 20."""
    import cetkmc
    bld = _check_build(build, L, n_steps, mode, bool(checkpoint_every or resume_from))
    n_sub = _thermal_substeps(thermal_substeps)
    _check_substeps(n_sub, mode == "A", thermal_updates)
    _check_scheme(thermal_scheme, mode == "A", thermal_updates)
    face_bc = _thermal_boundary(thermal_boundary, L, temp, mode == "A", thermal_scheme, thermal_updates)
    remelt_thr = _remelt_threshold(remelt)
    _check_remelt(remelt_thr, mode == "A", origin_metrics, thermal_updates)
    _check_solid(solid_metrics, solid_every, bool(checkpoint_every or resume_from))
    _check_origin(origin_metrics, bool(checkpoint_every or resume_from))
    if mode not in ("A", "B"):
        raise ValueError("mode must be 'A' (exact, one event per sweep) or 'B' (super-steps)")
    if laser is not None:
        laser = _check_laser(laser)
        if mode != "A":
            raise ValueError("laser needs mode 'A' (the super-step engine has no laser option here)")
        if checkpoint_every or resume_from:
            raise ValueError("laser cannot be combined with checkpoint_every / resume_from (a checkpoint does not carry prev_state)")
        if not thermal_updates:
            raise ValueError("laser needs thermal_updates=True (the source acts through the temperature update)")
        _check_beam_route(laser, thermal_scheme, L)
    if thermal_cadence not in ("events", "supersteps"):
        raise ValueError("thermal_cadence must be 'events' or 'supersteps'")
    local_events = int(local_events)
    if local_events:
        if mode != "B" or box != 8 or L % 8:
            raise ValueError("local_events needs mode 'B' with box 8 dividing L")
        if not 1 <= local_events <= 64 or not float(local_horizon) > 0.0:
            raise ValueError("local_events must be 1..64 and local_horizon > 0")
    run_seed = RANDOM_SEED if seed is None else int(seed)
    metrics_every = int(metrics_every)

    output_dir = f"outputs/{output_prefix}"
    os.makedirs(output_dir, exist_ok=True)
    ckpt = None
    if resume_from:
        ckpt = load_checkpoint(resume_from)
        state, theta, phi, T = ckpt["state"], ckpt["theta"], ckpt["phi"], ckpt["T"]
        atom_type = state.copy()
        defects_mask = ckpt["defects"]
    else:
        np.random.seed(run_seed)
        random.seed(run_seed)
        state, theta, phi, T, atom_type = initialize_lattice(
            lattice_size=L, n_seeds=n_seeds, T_sub=temp, impurity_c=impurity_c)
        defects_mask, defect_density = introduce_defects(state, atom_type, T, apply_to_state=False)

    nu_dep_eff = NU_DEP if nu_dep is None else float(nu_dep)
    G, R, R_phys, G_over_R_phys = _nominal_gr(L, nu_dep_eff)

    params = cetkmc.default_params(impurity_c)
    params.nu_dep = nu_dep_eff
    engine = cetkmc.Engine(L, impurity_c=impurity_c, params=params)
    engine.upload(state, theta, phi, T, defects_mask)
    remelt_off = (0, 0)            # passes and melted voxels of the run before the checkpoint it resumes from
    if remelt_thr is not None or (ckpt and "remelt" in ckpt["extra"]):
        ex = ckpt["extra"] if ckpt else {}
        if ckpt and ex.get("remelt") != remelt_thr:
            engine.close()
            raise ValueError(f"checkpoint was written by a run with remelt={ex.get('remelt', False)}, this call asks for {remelt_thr or False}")
        remelt_off = (int(ex.get("remelt_passes", 0)), int(ex.get("remelted", 0)))
    if ckpt and int(ckpt["extra"].get("thermal_substeps", 1)) != n_sub:
        engine.close()
        raise ValueError(f"checkpoint was written by a run with thermal_substeps={ckpt['extra'].get('thermal_substeps', 1)}, "
                         f"this call asks for {n_sub}")
    if ckpt and ckpt["extra"].get("thermal_scheme", "explicit") != thermal_scheme:
        engine.close()
        raise ValueError(f"checkpoint was written by a run with thermal_scheme={ckpt['extra'].get('thermal_scheme', 'explicit')!r}, "
                         f"this call asks for {thermal_scheme!r}")
    if ckpt and ckpt["extra"].get("thermal_bc") != face_bc:
        engine.close()
        raise ValueError(f"checkpoint was written by a run with thermal_boundary={ckpt['extra'].get('thermal_bc')!r}, "
                         f"this call asks for {face_bc!r}")
    _apply_thermal_options(engine, n_sub, thermal_scheme, face_bc, remelt_thr)
    beam = laser is not None and "path" in laser
    if beam:
        engine.set_beam(_beam_table_of_layer(laser, L, 0, n_steps) if bld else _beam_table_of(laser, L, n_steps))
    n_flagged = int(np.sum(defects_mask))
    if mode == "B" and not (box == L or (box in (8, 10, 12, 14, 16) and L % box == 0)):
        engine.close()
        raise ValueError("mode 'B': box must be even, 8..16, and divide L (or equal L: single domain)")

    total_time = 0.0
    min_margin = 1.0
    metrics_data = []
    cet_detected = False
    step = -1
    next_step = 0
    nuc_offset = 0
    layer_planes = texture_planes = grain_rows = solid_grain_rows = None
    solid_planes = []
    solid = dict(remelted=0, stamp=0, thermal=0)      # running n_cleared; step count and temperature updates at the last map update
    solid_scales = cetkmc.engine.default_solid_scales()
    if solid_metrics:
        engine.solid_begin()
    origin_planes, origin_grain_rows = [], None
    if origin_metrics:
        engine.origin_begin()

    def solid_update(stamp, thermal_now):
        """the map update at ``stamp`` executed steps, ``thermal_now`` temperature updates issued so far"""
        info = engine.solid_update(stamp, max(1, thermal_now - solid["thermal"]) * THERMAL_DT)
        solid.update(remelted=solid["remelted"] + info["n_cleared"], stamp=stamp, thermal=thermal_now)
    if ckpt:
        total_time, metrics_data, cet_detected = ckpt["total_time"], ckpt["metrics_data"], ckpt["cet_detected"]
        next_step, nuc_offset = ckpt["next_step"], ckpt["nucleation_count"]
        step = next_step - 1
    def metrics_row(step, refresh_defects):
        """kmc_simulation.py:335-389 for the lattice as it stands after event index `step` -- WITHOUT moving the lattice: the
        defect mask is refreshed from the carbon sites only, grains are clustered and species counted on the GPU."""
        nonlocal n_flagged, cet_detected, layer_planes, texture_planes, grain_rows, solid_grain_rows, origin_grain_rows
        if refresh_defects:
            n_flagged, _ = refresh_defects_device(engine)       # kmc_simulation.py:335-338
        cl = engine.clusters(0.5, labels=True)
        row = _metrics_row(cl, engine.species_counts(), engine.nucleation_count(), L, step,
                           total_time, n_flagged, nuc_offset, cet_detected, G, R, R_phys, G_over_R_phys)
        cet_detected = row["CET_Detected"]
        if front_metrics:
            _add_front_columns(row, engine.front_stats(), L, metrics_data[-1] if metrics_data else None)
        if layer_metrics:               # from the clustering of this row: no second clustering, no label download
            layer_planes = _add_layer_columns(row, engine.layer_profile(recluster=False), L)
        if texture_metrics:
            texture_planes = _add_texture_columns(row, engine.texture_profile(recluster=False))
        if grain_metrics:
            grain_rows = _add_grain_columns(row, engine.grain_table(recluster=False))
        if solid_metrics:
            planes, solid_grain_rows = _add_solid_columns(
                row, engine.solid_profile(solid_scales, grains=grain_metrics, recluster=False), solid_scales, solid["remelted"], cl)
            solid_planes.append(planes)
        if origin_metrics:
            # grain records from the row's own clustering (the grain columns need them); their table only with grain_metrics
            planes, g_rows = _add_origin_columns(row, engine.origin_profile(grains=True, recluster=False), engine.origin_census())
            origin_grain_rows = g_rows if grain_metrics else None
            origin_planes.append(planes)
        if remelt_thr is not None:
            _add_remelt_columns(row, engine.remelt_info(), remelt_off)
        if bld:
            row["Layer"] = layer
            plane_tables.clear()
            if layer_metrics:
                plane_tables["layer"] = layer_planes
            if solid_metrics:
                plane_tables["solid"] = solid_planes[-1]
            if origin_metrics:
                plane_tables["origin"] = origin_planes[-1]
        metrics_data.append(row)
        _print_row(step, row)

    def checkpoint(at, extra=None):
        if remelt_thr is not None:       # (only then: the checkpoints of every other run stay as they were)
            info = engine.remelt_info()
            extra = dict(extra or {}, remelt=remelt_thr, remelt_passes=remelt_off[0] + info["passes"], remelted=remelt_off[1] + info["n_melted"])
        if n_sub != 1:                   # (likewise)
            extra = dict(extra or {}, thermal_substeps=n_sub)
        if thermal_scheme != "explicit": # (likewise)
            extra = dict(extra or {}, thermal_scheme=thermal_scheme)
        if face_bc is not None:          # (likewise)
            extra = dict(extra or {}, thermal_bc=face_bc)
        save_checkpoint(os.path.join(output_dir, "checkpoint.npz"), engine.download(),
                        engine.download(state=False, theta=False, phi=False, T=False, defects=True)["defects"],
                        at, total_time, nuc_offset + engine.nucleation_count(), metrics_data, cet_detected, extra=extra)

    # a build: n_steps per layer, the global step index runs on; n_end = end of the current layer
    layer, n_layers, n_end = 0, (bld["layers"] if bld else 1), n_steps
    plane_tables, build_rows, retired, dropped = {}, [], 0, [0] * 6
    while mode == "A" and next_step < n_end:
        # next step after which the host has work: metrics (and, on multiples of
        # metrics_every, the defect-mask refresh) -- kmc_simulation.py:335-341
        stop = next_step if next_step % metrics_every == 0 else \
            min((next_step // metrics_every + 1) * metrics_every, n_end - 1)
        stop = min(stop, n_end - 1)
        if checkpoint_every > 0:      # also stop right before every checkpoint boundary
            stop = min(stop, (next_step // checkpoint_every + 1) * checkpoint_every - 1)
        if solid_metrics:             # ... and right before every map update
            stop = min(stop, (next_step // solid_every + 1) * solid_every - 1)
        done, terminated, last_total, dts, margin = _advance_to(engine, next_step, stop, L, defect_fraction, incremental=incremental,
                                                                 thermal_mode=1 if thermal_updates else 0, laser=laser)
        for dt in dts:
            total_time += dt
        min_margin = min(min_margin, margin)
        if terminated:
            step = next_step + done
            print(f"Terminating at step {step}: no valid events (rate={last_total:.2e})")
            break
        step = stop
        next_step = stop + 1

        if solid_metrics and next_step % solid_every == 0:
            solid_update(next_step, _updates_between(0, next_step) if thermal_updates else 0)
        is_metric_step = (step % metrics_every == 0) or (step == n_end - 1)
        if not is_metric_step:        # a pure checkpoint (or map-update) stop
            if checkpoint_every > 0:
                checkpoint(next_step)
            continue
        metrics_row(step, step % metrics_every == 0)
        if checkpoint_every > 0 and next_step % checkpoint_every == 0:
            checkpoint(next_step)
        if bld and next_step == n_end and layer < n_layers - 1:
            # the layer is complete and its row is written: the planes about to leave go to build_layers.csv, the part is
            # lowered by a layer on the device, and the next layer's scan begins
            h = bld["thickness"]
            if plane_tables:
                build_rows += _retired_planes(plane_tables, h, layer, retired)
            info = engine.shift((-h, 0, 0), fill_state=bld["state"], fill_T=bld["T"], T_mode="value")
            dropped = [a + b for a, b in zip(dropped, info["dropped"])]
            retired, layer, n_end = retired + h, layer + 1, n_end + n_steps
            if beam:
                engine.set_beam(_beam_table_of_layer(laser, L, layer, n_steps))
    # the planes that remain, from the last metrics row -- unless the run terminated behind that row: then the lattice has moved on
    # since, the file ends with the retired planes and last_run_info["build"]["complete"] says so
    build_complete = bool(bld) and next_step == n_end and layer == n_layers - 1
    if bld and plane_tables and build_complete:
        build_rows += _retired_planes(plane_tables, L, layer, retired)

    if mode == "B":
        # Super-step loop.  executed = events executed so far = index of the next event; g = super-step index (octant
        # g % 8, keys the counter uniforms together with run_seed).
        nbx = L // box if (box and L % box == 0) else 1
        d_max = 1 if box == L else nbx ** 3                       # events per super-step at most
        if local_events:
            d_max *= local_events
        executed, g, thermal_done = 0, 0, 0
        horizon_time, capped_boxes = 0.0, 0
        mb_cfg = dict(mode="B", box=int(box), seed=run_seed, null_events=bool(null_events), thermal_cadence=thermal_cadence,
                      thermal_updates=bool(thermal_updates))
        if local_events:        # (only then: the checkpoints of every other run stay as they were)
            mb_cfg.update(local_events=local_events, local_horizon=float(local_horizon))
        if ckpt:
            ex = ckpt["extra"]
            if {k: ex.get(k) for k in mb_cfg} != mb_cfg or ("local_events" in ex) != bool(local_events):
                engine.close()
                raise ValueError(f"checkpoint was written by a run with {ex}, this call asks for {mb_cfg}")
            executed, g, thermal_done = next_step, int(ex["superstep"]), int(ex["thermal_done"])
            horizon_time, capped_boxes = float(ex.get("horizon_time", 0.0)), int(ex.get("capped_boxes", 0))
        by_events = thermal_cadence == "events" and thermal_updates
        engine_thermal = 0
        while executed < n_steps:
            # super-steps until (at the earliest) the next metrics / checkpoint boundary or the end: a super-step executes
            # <= d_max events (a row is due once executed - 1 reaches the next multiple of metrics_every)
            boundary = min(((executed - 1) // metrics_every + 1) * metrics_every + 1, n_steps)
            if checkpoint_every > 0:
                boundary = min(boundary, (executed // checkpoint_every + 1) * checkpoint_every)
            if solid_metrics:
                boundary = min(boundary, (executed // solid_every + 1) * solid_every)
            nb = max(1, (boundary - executed) // d_max)
            if by_events:
                # kmc_simulation.py:248-250: event index e is preceded by e // 20 + 1 temperature updates; the super-step's
                # events all see the field of its first event (the lattice and T are frozen within a super-step)
                nb = 1
                due = executed // THERMAL_EVERY + 1
                for _ in range(due - thermal_done):
                    engine.thermal_cet(THERMAL_DT, scrub_nan=True)
                thermal_done = due
            engine_mode = 0 if (by_events or not thermal_updates) else 1
            if local_events:
                r = engine.run_supersteps_local(g, nb, defect_fraction, run_seed, local_events, float(local_horizon),
                                                thermal_mode=engine_mode, thermal_dt=THERMAL_DT)
                for s in range(r["done"]):
                    horizon_time += float(r["horizon"][s]) / 8.0
                    capped_boxes += int(r["n_capped"][s])
            else:
                r = engine.run_supersteps(g, nb, box, defect_fraction, run_seed, thermal_mode=engine_mode,
                                          thermal_dt=THERMAL_DT, null_events=null_events)
            before = executed
            for s in range(r["done"]):
                executed += int(r["n_exec"][s])
                total_time += int(r["n_exec"][s]) * float(r["dt_event"][s])
            if not by_events and thermal_updates:      # (the engine updates T at every 20th super-step)
                engine_thermal += _updates_between(g, g + r["done"])
            g += r["done"]
            step = executed - 1
            if r["status"] == 1:
                print(f"Terminating at step {executed}: no valid events (rate={float(r['totals'][r['done']]):.2e})")
                break
            if solid_metrics and executed // solid_every > before // solid_every:
                solid_update(executed, thermal_done if by_events else engine_thermal)
            crossed = (executed - 1) // metrics_every > (before - 1) // metrics_every
            if crossed or executed >= n_steps:
                metrics_row(step, crossed)
            if checkpoint_every > 0 and executed // checkpoint_every > before // checkpoint_every:
                # after the row of this super-step: a resumed run continues with the next super-step
                extra = dict(mb_cfg, superstep=g, thermal_done=thermal_done)
                if local_events:
                    extra.update(horizon_time=horizon_time, capped_boxes=capped_boxes)
                checkpoint(executed, extra)
        next_step = executed

    if metrics_data:
        print(f"Metrics saved to {_write_metrics(output_prefix, metrics_data)}")
    if layer_planes is not None:
        _write_layers_csv(os.path.join(output_dir, "layers.csv"), layer_planes)
    if texture_planes is not None:
        _write_texture_csv(os.path.join(output_dir, "texture.csv"), texture_planes)
    if grain_rows is not None:
        _write_grains_csv(os.path.join(output_dir, "grains.csv"), grain_rows)
    if solid_planes:
        _write_solid_csv(os.path.join(output_dir, "solid_layers.csv"), solid_planes)
    if solid_grain_rows is not None:
        _write_solid_csv(os.path.join(output_dir, "solid_grains.csv"), [solid_grain_rows])
    if origin_planes:
        _write_origin_csv(os.path.join(output_dir, "origin_layers.csv"), origin_planes)
    if origin_grain_rows is not None:
        _write_origin_csv(os.path.join(output_dir, "origin_grains.csv"), [origin_grain_rows])
    if bld and build_rows:
        pd.DataFrame(build_rows).to_csv(os.path.join(output_dir, "build_layers.csv"), index=False)

    fields = engine.download()
    state, theta, phi = fields["state"], fields["theta"], fields["phi"]
    atom_type = state.copy()
    remelted = remelt_off[1] + engine.remelt_info()["n_melted"] if remelt_thr is not None else None
    beam_report = dict(engine.beam_info(), path=dict(laser["path"]), depth=int(laser.get("depth", 1))) if beam else None
    engine.close()
    last_run_info.clear()
    last_run_info.update(mode=mode, min_margin=min_margin if mode == "A" else None, executed_events=step + 1, thermal_substeps=n_sub,
                         thermal_scheme=thermal_scheme, thermal_boundary=face_bc)
    if remelt_thr is not None:
        last_run_info.update(remelted=remelted)
    if beam:
        last_run_info.update(beam=beam_report)
    if local_events:
        last_run_info.update(horizon_time=horizon_time, capped_boxes=capped_boxes)
    if bld:
        last_run_info.update(build=dict(layers=n_layers, thickness=bld["thickness"], retired_planes=retired, dropped=dropped,
                                         complete=build_complete))
    if mode == "A" and min_margin < MARGIN_WARN:
        print(f"Note: smallest selection margin {min_margin:.2e} < {MARGIN_WARN:.0e} of the total rate -- a pick this close to an "
              "event boundary may differ from the reference's sequential scan")
    print(f"Completed {step + 1} steps in {total_time:.2e} s")
    return state, atom_type, total_time, theta, phi


# ---- replica ensembles: many independent runs in the same launches -----------------------------
_C_SITE = 3                 # carbon state (defects.py: only carbon sites can become defects)
ENSEMBLE_KEYS = ("temp", "defect_fraction", "n_seeds", "impurity_c", "output_prefix", "nu_dep", "seed", "laser", "remelt")
_RUN_DEFAULTS = dict(temp=T_SUB, defect_fraction=0.0, n_seeds=5, impurity_c=0.0, output_prefix="cet_run", nu_dep=None, seed=None,
                     laser=None, remelt=False)
# per-replica generators and counters of the last run_kmc_ensemble call (the return tuples have no room for them):
# random_state / np_state (where run_kmc would have left the global generators), executed_events, min_margin
last_ensemble_info = []


def _ensemble_configs(configs, L, n_steps, rng, metrics_every, thermal_updates=True, origin_metrics=False):
    """Argument validation of run_kmc_ensemble (before any device call); returns the completed per-replica configs."""
    if rng not in ("reference", "counter"):
        raise ValueError("rng must be 'reference' (run_kmc's exact loop) or 'counter' (run_kmc mode 'B', box = L)")
    if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or not 1 <= int(L) <= 128:
        raise ValueError("ensembles cover 1 <= L <= 128")
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 0:
        raise ValueError("n_steps must be an integer >= 0")
    if int(metrics_every) < 1:
        raise ValueError("metrics_every must be >= 1")
    if not isinstance(configs, (list, tuple)) or len(configs) < 1:
        raise ValueError("configs must be a non-empty list of dicts (one per replica)")
    out = []
    for i, c in enumerate(configs):
        if not isinstance(c, dict):
            raise ValueError(f"configs[{i}] is not a dict")
        bad = set(c) - set(ENSEMBLE_KEYS)
        if bad:
            raise ValueError(f"configs[{i}]: unknown keys {sorted(bad)} (allowed: {', '.join(ENSEMBLE_KEYS)})")
        d = dict(_RUN_DEFAULTS, **c)
        if not (float(d["defect_fraction"]) >= 0.0):
            raise ValueError(f"configs[{i}]: defect_fraction must be >= 0")
        if d["laser"] is not None:
            d["laser"] = _check_laser(d["laser"], f"configs[{i}]['laser']")
        d["remelt"] = _remelt_threshold(d["remelt"], f"configs[{i}]['remelt']")
        out.append(d)
    if len({d["remelt"] for d in out}) != 1:
        raise ValueError("the 'remelt' setting must be the same in every config (it is shared by the ensemble)")
    _check_remelt(out[0]["remelt"], rng == "reference", origin_metrics, thermal_updates)
    lasers = [d["laser"] is not None for d in out]
    if any(lasers):
        # the thermal mode belongs to the call, and a laser of zero power does not give the bits of the diffusion-only update
        if not all(lasers):
            raise ValueError("either every config has a laser or none has (the thermal mode is shared by the ensemble)")
        if not thermal_updates:
            raise ValueError("laser needs thermal_updates=True (the source acts through the temperature update)")
        if len({bool(d["laser"].get("latent", True)) for d in out}) != 1:
            raise ValueError("the lasers' 'latent' setting must be the same in every config (it is shared by the ensemble)")
        if len({"path" in d["laser"] for d in out}) != 1:
            raise ValueError("either every laser has a 'path' (the beam route) or none has (the route is shared by the ensemble)")
        if len({int(d["laser"].get("depth", 1)) for d in out}) != 1:
            raise ValueError("the lasers' 'depth' must be the same in every config (the ensemble's beam tables share it)")
    if rng == "reference" and len(out) * (int(L) * int(L) + 2) > _MAX_STREAM_DOUBLES:
        raise ValueError(f"rng='reference': R * (L*L + 2) must stay within {_MAX_STREAM_DOUBLES} pre-drawn doubles per step "
                         "(split the ensemble)")
    prefixes = [d["output_prefix"] for d in out]
    if len(set(prefixes)) != len(prefixes):
        raise ValueError("every replica needs its own output_prefix (outputs/<prefix>/metrics.csv)")
    return out


class _GlobalRNG:
    """Swaps a replica's private generator states into the global ``random`` / ``np.random`` for a host call that draws
    from them (initialize_lattice, introduce_defects, refresh_defects_device), and takes the advanced states back."""

    def __init__(self, py_state, np_state):
        self.py, self.np = py_state, np_state

    def __enter__(self):
        random.setstate(self.py)
        np.random.set_state(self.np)
        return self

    def __exit__(self, *exc):
        self.py, self.np = random.getstate(), np.random.get_state()
        return False


def _replica_prefix(cfg, L):
    """run_kmc's host prefix (kmc_simulation.py:222-227) for one replica, under the global generators: returns the initial
    fields, the defect mask and the generator states it leaves behind."""
    run_seed = RANDOM_SEED if cfg["seed"] is None else int(cfg["seed"])
    np.random.seed(run_seed)
    random.seed(run_seed)
    state, theta, phi, T, atom_type = initialize_lattice(
        lattice_size=L, n_seeds=cfg["n_seeds"], T_sub=cfg["temp"], impurity_c=cfg["impurity_c"])
    defects_mask, _ = introduce_defects(state, atom_type, T, apply_to_state=False)
    return dict(state=state, theta=theta, phi=phi, T=T, defects=defects_mask, seed=run_seed,
                py_state=random.getstate(), np_state=np.random.get_state())


def run_kmc_ensemble(configs, L, n_steps, *, rng="reference", metrics_every=METRIC_UPDATE_STEP, thermal_updates=True,
                     front_metrics=False, layer_metrics=False, texture_metrics=False, grain_metrics=False, solid_metrics=False,
                     solid_every=20, origin_metrics=False, thermal_substeps=1, thermal_scheme="explicit", thermal_boundary=None):
    """Many independent run_kmc calls of the same L and n_steps stepped together on one GPU (cetkmc.Ensemble).

    ``configs``: one dict per replica with run_kmc's per-run arguments (temp, defect_fraction, n_seeds, impurity_c,
    output_prefix, nu_dep, seed, laser, remelt).  ``remelt`` (run_kmc's option of that name: rows gain ``RemeltPasses`` and
    ``RemeltedVoxels``; ``last_ensemble_info[r]["remelted"]``) is shared like the lasers' ``latent``: the same in every config,
    ``rng="reference"`` only.  ``laser`` (run_kmc's laser dict): either every config has one or none has, with
    the same ``latent`` setting; configs with equal dicts share one set of source planes on the device.  Returns one run_kmc return tuple per replica and writes each replica's
    ``outputs/<prefix>/metrics.csv`` and ``metrics_<tag>.csv``.

    ``rng="reference"``: replica r equals ``run_kmc(L=L, n_steps=n_steps, **configs[r])`` bit for bit (arrays, total_time,
    CSV; its private generators end where run_kmc leaves the global ones: ``last_ensemble_info``).
    ``rng="counter"``: replica r equals ``run_kmc(L=L, n_steps=n_steps, mode="B", box=L, thermal_cadence="supersteps",
    **configs[r])`` -- all-counter uniforms, the host draws nothing per step.  The caller's global generator states are
    restored on return.  One completion line is printed per replica (no per-row progress).
    ``front_metrics=True``: run_kmc's option of that name, from ONE batched cetkmc_ensemble_front_stats call per metrics row.
    ``layer_metrics=True``: run_kmc's option of that name (columns and ``layers.csv`` of every replica), from ONE batched
    cetkmc_ensemble_layer_profile call per metrics row on the row's own analysis.
    ``texture_metrics=True``: run_kmc's option of that name (columns and ``texture.csv`` of every replica), from ONE batched
    cetkmc_ensemble_texture_profile call per metrics row on the row's own analysis.
    ``grain_metrics=True``: run_kmc's option of that name (columns and ``grains.csv`` of every replica), from ONE batched
    cetkmc_ensemble_grain_table call per metrics row on the row's own analysis.
    ``solid_metrics=True`` / ``solid_every``: run_kmc's options of that name (columns, ``solid_layers.csv`` and, with
    ``grain_metrics``, ``solid_grains.csv`` of every replica), from ONE batched cetkmc_ensemble_solid_update per multiple of
    ``solid_every`` steps and ONE batched cetkmc_ensemble_solid_profile per metrics row.
    ``origin_metrics=True``: run_kmc's option of that name (columns, ``origin_layers.csv`` and, with ``grain_metrics``,
    ``origin_grains.csv`` of every replica): every cetkmc_run_ensemble call folds the replicas' executed events into their
    origin maps in one launch, and every metrics row takes ONE batched cetkmc_ensemble_origin_profile and census.
    ``thermal_substeps``: run_kmc's option of that name, one value for all replicas (cetkmc_ensemble_set_thermal_substeps);
    ``rng="reference"`` only; ``last_ensemble_info[r]["thermal_substeps"]``.
    ``thermal_scheme``: run_kmc's option of that name, one value for all replicas (cetkmc_ensemble_set_thermal_scheme);
    ``rng="reference"`` only; ``last_ensemble_info[r]["thermal_scheme"]``.
    ``thermal_boundary``: run_kmc's option of that name, one value for all replicas (cetkmc_ensemble_set_thermal_boundary);
    ``"gradient"`` needs one ``temp`` for all; ``last_ensemble_info[r]["thermal_boundary"]``."""
    import cetkmc
    n_sub = _thermal_substeps(thermal_substeps)
    _check_substeps(n_sub, rng == "reference", thermal_updates)
    _check_scheme(thermal_scheme, rng == "reference", thermal_updates,
                  needs="rng='reference' (the counter mode steps through the super-step engine, whose updates are explicit)")
    _check_solid(solid_metrics, solid_every, False)
    cfgs = _ensemble_configs(configs, L, n_steps, rng, metrics_every, thermal_updates, origin_metrics)
    for c in cfgs:
        _check_beam_route(c["laser"], thermal_scheme, int(L))
    if thermal_boundary == "gradient" and len({float(c["temp"]) for c in cfgs}) != 1:
        raise ValueError("thermal_boundary='gradient' needs one temp for all replicas (the ensemble shares one boundary)")
    boundary = _thermal_boundary(thermal_boundary, int(L), cfgs[0]["temp"], rng == "reference", thermal_scheme, thermal_updates,
                                 needs="rng='reference' (the counter mode steps through the super-step engine, whose updates are explicit)")
    L, n_steps, me, R = int(L), int(n_steps), int(metrics_every), len(cfgs)
    caller_py, caller_np = random.getstate(), np.random.get_state()
    ens = None
    try:
        pre = [_replica_prefix(c, L) for c in cfgs]
        gens = [_GlobalRNG(p["py_state"], p["np_state"]) for p in pre]
        params, geo = [], []
        for c in cfgs:
            p = cetkmc.default_params(c["impurity_c"])
            p.nu_dep = NU_DEP if c["nu_dep"] is None else float(c["nu_dep"])
            params.append(p)
            geo.append(_nominal_gr(L, p.nu_dep))
        ens = cetkmc.Ensemble(L, params)
        for r, p in enumerate(pre):
            ens.replica(r).upload(p["state"], p["theta"], p["phi"], p["T"], p["defects"])
        n_flagged = [int(np.sum(p["defects"])) for p in pre]
        for c in cfgs:
            os.makedirs(f"outputs/{c['output_prefix']}", exist_ok=True)
        df = np.array([float(c["defect_fraction"]) for c in cfgs])
        seeds = np.array([p["seed"] for p in pre], dtype=np.uint64)
        per = [3 if d > 0.0 else 2 for d in df]
        per_step = L * L + 2
        alive = [True] * R
        total_time = [0.0] * R
        last_step = [-1] * R
        min_margin = [1.0] * R
        metrics = [[] for _ in range(R)]
        cet = [False] * R
        layer_planes = [None] * R
        texture_planes = [None] * R
        grain_rows = [None] * R
        solid_planes = [[] for _ in range(R)]
        solid_grain_rows = [None] * R
        remelted = np.zeros(R, np.int64)
        solid_thermal = 0                    # temperature updates issued before the last map update
        solid_scales = cetkmc.engine.default_solid_scales()
        if solid_metrics:
            ens.solid_begin()
        origin_planes = [[] for _ in range(R)]
        origin_grain_rows = [None] * R
        if origin_metrics:
            ens.origin_begin()
        remelt_thr = cfgs[0]["remelt"]
        _apply_thermal_options(ens, n_sub, thermal_scheme, boundary, remelt_thr)
        thermal_mode = 1 if thermal_updates else 0
        # laser configs: replicas with equal scans (the seeds of one map point) share a plane set
        scans, q_set, use_latent = [], None, True
        if cfgs[0]["laser"] is not None:
            thermal_mode, q_set = 2, np.zeros(R, np.int32)
            use_latent = bool(cfgs[0]["laser"].get("latent", True))
            for r, c in enumerate(cfgs):
                if c["laser"] not in scans:
                    scans.append(c["laser"])
                q_set[r] = scans.index(c["laser"])
        beam = bool(scans) and "path" in scans[0]
        if beam:                # one table per distinct laser dict, on the device for the whole run
            ens.set_beam([_beam_table_of(z, L, n_steps) for z in scans], q_set)

        def laser_kw(s0, n):
            if not scans:
                return {}
            if beam:
                return dict(use_latent=use_latent)
            q = np.stack([laser_scan_planes(L, z, s0, n) for z in scans])
            return dict(q_planes=q if q.shape[1] else None, q_set=q_set, use_latent=use_latent)
        cap = _MAX_STREAM_DOUBLES // (R * per_step) if rng == "reference" else 4096
        next_step = 0
        while next_step < n_steps and any(alive):
            # the same stops as run_kmc: every metrics row (and the defect refresh on its multiples) -- kmc_simulation.py:335-341
            stop = next_step if next_step % me == 0 else min((next_step // me + 1) * me, n_steps - 1)
            stop = min(stop, n_steps - 1)
            s0 = next_step
            while s0 <= stop and any(alive):
                n = min(stop - s0 + 1, cap)
                if solid_metrics:            # the batch ends right before the next map update
                    n = min(n, (s0 // solid_every + 1) * solid_every - s0)
                if rng == "reference":
                    u_pick = np.zeros((R, n))
                    u_def = np.zeros((R, n)) if np.any(df > 0.0) else None
                    u_np = np.zeros((R, n * per_step))
                    draws, saved = [None] * R, [None] * R
                    for r in range(R):
                        if not alive[r]:
                            continue
                        with gens[r]:          # from the replica's generators
                            saved[r], draws[r], u_np[r] = _draw_uniforms(per[r], n, per_step)
                        u_pick[r] = draws[r][:, 0]
                        if per[r] == 3:
                            u_def[r] = draws[r][:, 1]
                    res = ens.run(s0, n, df, u_pick, u_def, u_np, rng_mode=0, thermal_mode=thermal_mode, thermal_dt=THERMAL_DT,
                                  **laser_kw(s0, n))
                else:
                    res = ens.run(s0, n, df, rng_mode=2, seeds=seeds, thermal_mode=thermal_mode, thermal_dt=THERMAL_DT,
                                  **laser_kw(s0, n))
                for r in range(R):
                    if not alive[r]:
                        continue
                    done = int(res["done"][r])
                    min_margin[r] = min(min_margin[r], float(res["min_margin"][r]))
                    if rng == "reference":
                        with gens[r]:
                            _rewind_uniforms(saved[r], per[r], n, done, int(res["np_used"][r]))
                        for s in range(done):
                            total_time[r] += max(-np.log(max(1e-12, draws[r][s, per[r] - 1])) / res["totals"][r, s], 1e-12)
                    else:
                        for s in range(done):
                            total_time[r] += 1 * float(res["dt"][r, s])
                    if res["status"][r] == 1:
                        alive[r] = False
                        # the step index run_kmc reports: the terminating step in mode "A", the last executed one in mode "B"
                        last_step[r] = s0 + done if rng == "reference" else s0 + done - 1
                        print(f"[{cfgs[r]['output_prefix']}] terminating at step {s0 + done}: no valid events "
                              f"(rate={float(res['totals'][r, done]):.2e})")
                s0 += n
                if solid_metrics and s0 % solid_every == 0 and any(alive):
                    now = _updates_between(0, s0) if thermal_updates else 0
                    remelted += ens.solid_update(s0, max(1, now - solid_thermal) * THERMAL_DT)["n_cleared"]
                    solid_thermal = now
            # the metrics row of every live replica: one batched analysis (clustering, species and nucleation counts,
            # carbon gather) and one batched defect scatter -- launches independent of R
            if not any(alive):
                break
            refresh = stop % me == 0
            an = ens.analyze(0.5, species=_C_SITE if refresh else -1, labels=True)
            if refresh:                  # kmc_simulation.py:335-338, the draws from each replica's own NumPy stream
                lists = [None] * R
                for r in range(R):
                    if alive[r]:
                        with gens[r]:
                            lists[r] = draw_defect_sites(*an[r]["gather"])
                        n_flagged[r] = int(len(lists[r]))
                ens.set_defects_sparse(lists)
            fs = ens.front_stats() if front_metrics else None
            lp = ens.layer_profile(recluster=False) if layer_metrics else None
            tp = ens.texture_profile(recluster=False) if texture_metrics else None
            gt = ens.grain_table(recluster=False) if grain_metrics else None
            sp = ens.solid_profile(solid_scales, grains=grain_metrics, recluster=False) if solid_metrics else None
            op = ens.origin_profile(grains=True, recluster=False) if origin_metrics else None
            oc = ens.origin_census() if origin_metrics else None
            ri = ens.remelt_info() if remelt_thr is not None else None
            for r in range(R):
                if not alive[r]:
                    continue
                last_step[r] = stop
                G, Rg, R_phys, GoR = geo[r]
                row = _metrics_row(an[r]["clusters"], an[r]["counts"], an[r]["nucleation_count"], L, stop, total_time[r],
                                   n_flagged[r], 0, cet[r], G, Rg, R_phys, GoR)
                cet[r] = row["CET_Detected"]
                if fs is not None:
                    _add_front_columns(row, {k: v[r] for k, v in fs.items()}, L, metrics[r][-1] if metrics[r] else None)
                if lp is not None:
                    layer_planes[r] = _add_layer_columns(row, {k: v[r] for k, v in lp.items()}, L)
                if tp is not None:
                    texture_planes[r] = _add_texture_columns(
                        row, {k: (v[r] if k in ("gb_hist", "pole_hist", "bad") else v) for k, v in tp.items()})
                if gt is not None:
                    grain_rows[r] = _add_grain_columns(row, gt[r])
                if sp is not None:
                    prof = dict(layers={k: v[r] for k, v in sp["layers"].items()}, grains=sp["grains"][r] if sp["grains"] is not None else None)
                    planes, solid_grain_rows[r] = _add_solid_columns(row, prof, solid_scales, int(remelted[r]), an[r]["clusters"])
                    solid_planes[r].append(planes)
                if op is not None:
                    prof = dict(layers={k: v[r] for k, v in op["layers"].items()}, grains=op["grains"][r] if op["grains"] is not None else None)
                    planes, g_rows = _add_origin_columns(row, prof, oc[r])
                    origin_grain_rows[r] = g_rows if grain_metrics else None
                    origin_planes[r].append(planes)
                if ri is not None:
                    _add_remelt_columns(row, ri[r])
                metrics[r].append(row)
            next_step = stop + 1

        out = []
        last_ensemble_info.clear()
        ri = ens.remelt_info() if remelt_thr is not None else None
        for r, c in enumerate(cfgs):
            if metrics[r]:
                _write_metrics(c["output_prefix"], metrics[r])
            if layer_planes[r] is not None:
                _write_layers_csv(os.path.join(f"outputs/{c['output_prefix']}", "layers.csv"), layer_planes[r])
            if texture_planes[r] is not None:
                _write_texture_csv(os.path.join(f"outputs/{c['output_prefix']}", "texture.csv"), texture_planes[r])
            if grain_rows[r] is not None:
                _write_grains_csv(os.path.join(f"outputs/{c['output_prefix']}", "grains.csv"), grain_rows[r])
            if solid_planes[r]:
                _write_solid_csv(os.path.join(f"outputs/{c['output_prefix']}", "solid_layers.csv"), solid_planes[r])
            if solid_grain_rows[r] is not None:
                _write_solid_csv(os.path.join(f"outputs/{c['output_prefix']}", "solid_grains.csv"), [solid_grain_rows[r]])
            if origin_planes[r]:
                _write_origin_csv(os.path.join(f"outputs/{c['output_prefix']}", "origin_layers.csv"), origin_planes[r])
            if origin_grain_rows[r] is not None:
                _write_origin_csv(os.path.join(f"outputs/{c['output_prefix']}", "origin_grains.csv"), [origin_grain_rows[r]])
            fields = ens.replica(r).download()
            state = fields["state"]
            out.append((state, state.copy(), total_time[r], fields["theta"], fields["phi"]))
            last_ensemble_info.append(dict(random_state=gens[r].py, np_state=gens[r].np, executed_events=last_step[r] + 1,
                                           min_margin=min_margin[r] if rng == "reference" else None,
                                           thermal_substeps=n_sub, thermal_scheme=thermal_scheme, thermal_boundary=boundary,
                                           **({"remelted": ri[r]["n_melted"]} if ri is not None else {})))
            print(f"[{c['output_prefix']}] completed {last_step[r] + 1} steps in {total_time[r]:.2e} s")
        return out
    finally:
        if ens is not None:
            ens.close()
        random.setstate(caller_py)
        np.random.set_state(caller_np)
