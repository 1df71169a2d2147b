"""Carbon-level sweep driver (equivalent of the reference ``main.py:17-108``).

For each carbon level: save the initial lattice, run the GPU KMC (kmc_simulation.run_kmc), read
back ``metrics.csv`` and classify the final microstructure.  Plotting is optional (matplotlib is
only imported when ``--plots`` is given); the reference's visualization / graphs modules are
outside the accelerated path and are not part of this package.

    python main.py [--L 30] [--steps 20000] [--levels 0.0 0.1 0.2] [--plots] [--mode B --box 8]
    python main.py --ensemble [--rng counter]     # all carbon levels as one replica ensemble (run_kmc_ensemble)
    python main.py --front                        # every metrics.csv with the measured front columns (run_kmc front_metrics)
    python main.py --layers                       # layer columns in every metrics.csv and a layers.csv per level (run_kmc layer_metrics)
    python main.py --texture                      # texture columns in every metrics.csv and a texture.csv per level (run_kmc texture_metrics)
    python main.py --grains                       # grain columns in every metrics.csv and a grains.csv per level (run_kmc grain_metrics)
    python main.py --solid                        # solidification columns in every metrics.csv and a solid_layers.csv per level (run_kmc solid_metrics)
    python main.py --remelt [T]                   # remelting on the device: solid at or above T_MELT (or T) turns liquid (run_kmc remelt)
    python main.py --thermal-substeps N|stable    # sub-stepped temperature updates (run_kmc thermal_substeps; 'stable' = 17)
    python main.py --thermal-scheme implicit      # implicit temperature updates (run_kmc thermal_scheme)
    python main.py --thermal-scheme implicit --thermal-boundary gradient|sink    # held gradient / substrate sink (run_kmc thermal_boundary)
    python main.py --thermal-scheme implicit --laser-power P --scan raster|serpentine|line|diagonal [--scan-speed V] [--hatch H]
                   [--beam-depth D] [--penetration M]      # a laser scan path with a volumetric beam (run_kmc laser with a path)
    python main.py --build-layers N --layer-thickness H [--layer-T T]    # a build of N layers, --steps steps each (run_kmc build)
    python main.py --origin                       # origin columns in every metrics.csv and an origin_layers.csv per level (run_kmc origin_metrics)

``--ensemble`` with the default ``--rng reference`` writes the same files as the sequential run; ``--rng counter`` runs
every level like ``--mode B --box L`` with the super-step thermal cadence.
"""
import argparse
import os
import time

import numpy as np
import pandas as pd

from constants import DEFECT_PROB, LATTICE_SIZE, N_SEEDS, N_STEPS, T_SUB
from kmc_simulation import beam_laser, run_kmc, run_kmc_ensemble
from lattice_init import initialize_lattice, save_lattice
from metrics import detect_CET_transition


def check_args(L, n_steps, carbon_levels, ensemble, rng, run_kw):
    """Driver arguments, checked before any device call."""
    if rng not in ("reference", "counter"):
        raise ValueError("rng must be 'reference' or 'counter'")
    if ensemble:
        if run_kw:
            raise ValueError(f"--ensemble takes no run_kmc options ({sorted(run_kw)}): the RNG setting picks the mode")
        if not 1 <= L <= 128:
            raise ValueError("--ensemble covers 1 <= L <= 128")
        prefixes = [f"impurity_c_{int(c * 100)}" for c in carbon_levels]
        if len(set(prefixes)) != len(prefixes):
            raise ValueError("--ensemble: two carbon levels map to the same output directory")
    elif rng != "reference":
        raise ValueError("--rng counter needs --ensemble (the sequential equivalent is --mode B --box L)")
    if n_steps < 0 or not carbon_levels:
        raise ValueError("need n_steps >= 0 and at least one carbon level")


def main(L=LATTICE_SIZE, n_steps=N_STEPS, carbon_levels=(0.0, 0.1, 0.2), plots=False, ensemble=False, rng="reference", front=False,
         layers=False, texture=False, grains=False, solid=False, origin=False, remelt=False, thermal_substeps=1,
         thermal_scheme="explicit", thermal_boundary=None, scan=None, laser_power=None, scan_speed=1.0, hatch=None, beam_depth=1,
         penetration=None, **run_kw):
    check_args(L, n_steps, carbon_levels, ensemble, rng, run_kw)
    if scan is None and (hatch is not None or beam_depth != 1 or penetration is not None):
        raise ValueError("--hatch, --beam-depth and --penetration describe a --scan")
    if scan is not None and laser_power is None:
        raise ValueError("--scan needs --laser-power")
    # --scan: run_kmc's laser option with a path (the beam route; needs --thermal-scheme implicit), in every run / config
    lz = {"laser": beam_laser(laser_power, scan, scan_speed, hatch, beam_depth, penetration)} if scan is not None else {}
    rm = {"remelt": remelt} if remelt is not False and remelt is not None else {}      # --remelt: run_kmc's option / config key
    print("Starting KMC simulation for microstructure control...")
    t_start = time.time()
    summary = {"carbon_levels": [], "grain_sizes": [], "defect_densities": [], "aspect_ratios": []}
    ens_out, ens_t = None, 0.0
    fm = {"front_metrics": True} if front else {}     # --front: measured front columns in every metrics.csv (run_kmc)
    if thermal_substeps != 1:                         # --thermal-substeps: run_kmc's / run_kmc_ensemble's option of that name
        fm["thermal_substeps"] = thermal_substeps
    if thermal_scheme != "explicit":                  # --thermal-scheme: run_kmc's / run_kmc_ensemble's option of that name
        fm["thermal_scheme"] = thermal_scheme
    if thermal_boundary is not None:                  # --thermal-boundary: run_kmc's / run_kmc_ensemble's option of that name
        from thermal_solver import thermal_boundary as build_boundary
        fm["thermal_boundary"] = build_boundary(bottom=("fixed", T_SUB)) if thermal_boundary == "sink" else thermal_boundary
    if layers:                                        # --layers: layer columns and layers.csv (run_kmc layer_metrics)
        fm["layer_metrics"] = True
    if texture:                                       # --texture: texture columns and texture.csv (run_kmc texture_metrics)
        fm["texture_metrics"] = True
    if grains:                                        # --grains: grain columns and grains.csv (run_kmc grain_metrics)
        fm["grain_metrics"] = True
    if solid:                                         # --solid: solidification columns, solid_layers.csv (run_kmc solid_metrics)
        fm["solid_metrics"] = True
    if origin:                                        # --origin: origin columns, origin_layers.csv (run_kmc origin_metrics)
        fm["origin_metrics"] = True
    if ensemble:                  # every level in one replica ensemble; the per-level epilogue below reads its results
        for c in carbon_levels:
            prefix = f"impurity_c_{int(c * 100)}"
            os.makedirs(f"outputs/{prefix}/microstructures", exist_ok=True)
            init = initialize_lattice(lattice_size=L, n_seeds=N_SEEDS, T_sub=T_SUB, random_seed=42, impurity_c=c)
            save_lattice(*init[:4], init[4], prefix=f"outputs/{prefix}/init")
        t0 = time.time()
        ens_out = run_kmc_ensemble([dict(temp=T_SUB, defect_fraction=DEFECT_PROB, n_seeds=N_SEEDS, impurity_c=c,
                                         output_prefix=f"impurity_c_{int(c * 100)}", **rm, **lz) for c in carbon_levels], L, n_steps, rng=rng,
                                   **fm)
        ens_t = time.time() - t0
    for q, c in enumerate(carbon_levels):
        prefix = f"impurity_c_{int(c * 100)}"
        print(f"\nRunning simulation with {c * 100:.1f}% carbon")
        out_dir = f"outputs/{prefix}"
        os.makedirs(f"{out_dir}/microstructures", exist_ok=True)
        os.makedirs("output_images", exist_ok=True)
        t0 = time.time()
        if ens_out is None:
            init = initialize_lattice(lattice_size=L, n_seeds=N_SEEDS, T_sub=T_SUB, random_seed=42, impurity_c=c)
            save_lattice(*init[:4], init[4], prefix=f"{out_dir}/init")
            t0 = time.time()
            state, atom_type, total_time, theta, phi = run_kmc(L=L, n_steps=n_steps, temp=T_SUB, defect_fraction=DEFECT_PROB,
                                                               n_seeds=N_SEEDS, impurity_c=c, output_prefix=prefix, **run_kw, **fm, **rm, **lz)
        else:
            state, atom_type, total_time, theta, phi = ens_out[q]
            t0 -= ens_t / len(carbon_levels)
        t1 = time.time()
        csv_path = f"outputs/{prefix}/metrics.csv"
        status = "Undetected"
        if os.path.exists(csv_path):
            df = pd.read_csv(csv_path)
            if not df.empty:
                last = df.iloc[-1].to_dict()
                status = "Equiaxed" if detect_CET_transition(last) else "Columnar"
                summary["carbon_levels"].append(c)
                summary["grain_sizes"].append(last.get("AvgGrainSize", np.nan))
                summary["defect_densities"].append(last.get("DefectDensity", np.nan))
                summary["aspect_ratios"].append(last.get("AspectRatio", np.nan))
        else:
            print(f"Metrics file not found at {csv_path}")
        if plots:
            from lattice_init import visualize_initial_seeds
            visualize_initial_seeds(state, atom_type, title=f"Final State: {status} (C={c * 100:.0f}%)",
                                    filename=f"output_images/final_state_{prefix}.png")
        print(f"Completed {prefix} in {t1 - t0:.2f}s ({status})")
    print(f"\nTotal runtime: {time.time() - t_start:.2f} seconds")
    return summary


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=LATTICE_SIZE)
    ap.add_argument("--steps", type=int, default=N_STEPS)
    ap.add_argument("--levels", type=float, nargs="*", default=[0.0, 0.1, 0.2])
    ap.add_argument("--plots", action="store_true")
    ap.add_argument("--mode", choices=("A", "B"), default="A", help="A: exact loop (one event per sweep); B: super-steps")
    ap.add_argument("--box", type=int, default=8)
    ap.add_argument("--ensemble", action="store_true", help="run all carbon levels as one replica ensemble")
    ap.add_argument("--rng", choices=("reference", "counter"), default="reference",
                    help="--ensemble: reference streams (= the sequential run's files) or counter uniforms (= --mode B --box L)")
    ap.add_argument("--front", action="store_true", help="measured front columns (G, V, melt pool) in every metrics.csv")
    ap.add_argument("--layers", action="store_true", help="layer columns (CET height, intercepts, GB fractions) and layers.csv")
    ap.add_argument("--texture", action="store_true",
                    help="texture columns (boundary misorientation, low-angle / lateral shares, pole alignment) and texture.csv")
    ap.add_argument("--grains", action="store_true",
                    help="grain columns (moment-based elongation and inclination, columnar volume fraction, contacts) and grains.csv")
    ap.add_argument("--solid", action="store_true",
                    help="solidification map on the device: G, cooling rate and V at freezing in every metrics.csv, solid_layers.csv "
                         "(with --grains: solid_grains.csv)")
    ap.add_argument("--origin", action="store_true",
                    help="origin map on the device: voxels and grains by how they were filled (deposition, nucleation, attachment, "
                         "hop) in every metrics.csv, origin_layers.csv (with --grains: origin_grains.csv)")
    ap.add_argument("--remelt", type=float, nargs="?", const=True, default=False, metavar="T",
                    help="remelting on the device: behind every temperature update occupied voxels at or above T (default T_MELT) "
                         "become empty; RemeltPasses / RemeltedVoxels in every metrics.csv (mode A)")
    ap.add_argument("--thermal-substeps", type=lambda s: s if s == "stable" else int(s), default=1, metavar="N|stable",
                    help="every temperature update as N explicit steps of dt / N on the device ('stable': the smallest stable N, 17; "
                         "run_kmc thermal_substeps, mode A)")
    ap.add_argument("--thermal-scheme", choices=("explicit", "implicit"), default="explicit",
                    help="every temperature update as locally one-dimensional backward-Euler steps on the device, stable at any dt "
                         "(run_kmc thermal_scheme, mode A)")
    ap.add_argument("--thermal-boundary", choices=("gradient", "sink"), default=None,
                    help="with --thermal-scheme implicit: 'gradient' holds the imposed ramp (fixed faces at its next values), 'sink' "
                         "fixes T_SUB under the substrate face; every other face adiabatic (run_kmc thermal_boundary, mode A)")
    ap.add_argument("--scan", choices=("diagonal", "line", "raster", "serpentine"), default=None,
                    help="with --thermal-scheme implicit and --laser-power: the laser follows this scan path, its source built on the "
                         "device from a beam table (run_kmc laser with a path, mode A)")
    ap.add_argument("--laser-power", type=float, default=None, metavar="W", help="--scan: the beam's power [W]")
    ap.add_argument("--scan-speed", type=float, default=1.0, metavar="V", help="--scan: voxels per temperature update along a track")
    ap.add_argument("--hatch", type=float, default=None, metavar="H", help="--scan raster|serpentine: voxels between tracks")
    ap.add_argument("--beam-depth", type=int, default=1, metavar="D", help="--scan: planes from the top that absorb the beam")
    ap.add_argument("--penetration", type=float, default=None, metavar="M",
                    help="--beam-depth D > 1: e-folding depth of the absorption [m] (default: uniform over the D planes)")
    ap.add_argument("--local-events", type=int, default=0,
                    help="--mode B --box 8: local event loop, up to K events per box and super-step (run_kmc local_events)")
    ap.add_argument("--local-horizon", type=float, default=1.0, help="its time horizon in units of 1 / R_max (run_kmc local_horizon)")
    ap.add_argument("--build-layers", type=int, default=0, metavar="N",
                    help="a layer-by-layer build of N layers: --steps steps per layer, the part lowered on the device between them "
                         "(run_kmc build, mode A; with --layer-thickness)")
    ap.add_argument("--layer-thickness", type=int, default=None, metavar="H", help="--build-layers: planes per layer")
    ap.add_argument("--layer-T", type=float, default=None, metavar="T", help="--build-layers: temperature of a recoated layer (default T_SUB)")
    a = ap.parse_args()
    kw = dict(mode="B", box=a.box) if a.mode == "B" else {}
    if a.local_events:
        kw.update(local_events=a.local_events, local_horizon=a.local_horizon)
    if a.build_layers or a.layer_thickness is not None or a.layer_T is not None:
        if not a.build_layers or a.layer_thickness is None:
            ap.error("--build-layers N and --layer-thickness H come together (--layer-T is optional)")
        kw.update(build=dict(layers=a.build_layers, thickness=a.layer_thickness, **({"T": a.layer_T} if a.layer_T is not None else {})))
    main(a.L, a.steps, tuple(a.levels), a.plots, ensemble=a.ensemble, rng=a.rng, front=a.front, layers=a.layers, texture=a.texture,
         grains=a.grains, solid=a.solid, origin=a.origin, remelt=a.remelt, thermal_substeps=a.thermal_substeps,
         thermal_scheme=a.thermal_scheme, thermal_boundary=a.thermal_boundary, scan=a.scan, laser_power=a.laser_power,
         scan_speed=a.scan_speed, hatch=a.hatch, beam_depth=a.beam_depth, penetration=a.penetration, **kw)
