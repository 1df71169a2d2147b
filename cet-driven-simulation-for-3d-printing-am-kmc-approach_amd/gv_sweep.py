"""G-V sweep driver (BASELINE config 5: "full CET G-V sweep").

The reference only sweeps the carbon level (main.py:23); its thermal gradient G and growth velocity R are
constants derived in kmc_simulation.py:236-239 (G from T_SUB and the lattice height, R from NU_DEP).  This
driver varies both through the arguments the engine already takes: the substrate temperature ``temp`` of
run_kmc (initial T ramp, lattice_init.py:31) for G, and the deposition attempt frequency ``nu_dep`` for V, and
collects the CET classification of the last metrics row of every run into ``outputs/gv_sweep/gv_map.csv``.

    python gv_sweep.py [--L 30] [--steps 2000] [--temps 2800 3100 3400] [--nu-dep 2e12 2e13 2e14] [--carbon 0.2]
                       [--mode B --box 8 [--local-events K --local-horizon X]] [--seeds K] [--ensemble [--rng counter]]
                       [--laser-power P1,P2,... --scan-speed V1,V2,... [--laser-start J0]] [--front] [--layers] [--texture]
                       [--grains] [--solid] [--origin] [--remelt [T]] [--thermal-substeps N|stable] [--thermal-scheme implicit]

``--seeds K`` runs every point with the seeds RANDOM_SEED .. RANDOM_SEED + K - 1 (one gv_map.csv row per point and seed, with
a ``seed`` column when K > 1); ``--ensemble`` runs all of them as one replica ensemble (run_kmc_ensemble): with the default
``--rng reference`` it writes the files of the sequential run, ``--rng counter`` runs every point like ``--mode B --box L``
with the super-step thermal cadence.

``--laser-power`` and ``--scan-speed`` (both or neither) add two axes to the map: every point runs with run_kmc's ``laser``
option (a Gaussian beam of that power [W] moving by that many voxels per temperature update from ``--laser-start``), the
run directories carry ``_P<power>_S<speed>`` and gv_map.csv gains the columns ``power`` and ``speed``.  The seeds of one
point share the beam, so in an ensemble they share its source planes on the device.  Without the two flags the files are
what they were.

``--front`` measures the temperature gradient and the velocity of the growth front of every run on the device
(run_kmc's ``front_metrics``): every metrics.csv gains the front columns and gv_map.csv the columns ``G_front_K_per_m``,
``V_front_m_per_s`` and ``G_over_V_front`` from each run's last row, behind the nominal ``G_K_per_m`` / ``V_m_per_s`` /
``G_over_V`` (which are the same for every beam).  Without the flag the files are what they were.

``--layers`` measures the layer-resolved grain structure of every run on the device (run_kmc's ``layer_metrics``): every
metrics.csv gains the layer columns, every run directory a layers.csv, and gv_map.csv the columns ``CET_height_um`` and
``InterceptRatio`` from each run's last row (behind the front columns).  Without the flag the files are what they were.

``--texture`` measures the grain-boundary misorientation and pole histograms of every run on the device (run_kmc's
``texture_metrics``): every metrics.csv gains the texture columns, every run directory a texture.csv, and gv_map.csv the
columns ``GB_low_angle_frac`` and ``Pole_aligned_frac`` from each run's last row (behind the layer columns).  Without the
flag the files are what they were.

``--grains`` measures the per-grain table of every run on the device (run_kmc's ``grain_metrics``): every metrics.csv gains
the grain columns, every run directory a grains.csv, and gv_map.csv the columns ``Columnar_vol_frac`` and
``Grain_elong_mean`` from each run's last row (behind the texture columns).  Without the flag the files are what they were.

``--solid`` keeps a solidification map of every run on the device (run_kmc's ``solid_metrics``): every metrics.csv gains the
solidification columns, every run directory a solid_layers.csv (with ``--grains`` a solid_grains.csv), and gv_map.csv the
columns ``G_solid_K_per_m``, ``V_solid_m_per_s`` and ``G_over_V_solid`` -- gradient and isotherm velocity at the voxels WHEN
THEY FROZE -- from each run's last row (behind the grain columns).  Without the flag the files are what they were.

``--origin`` keeps an origin map of every run on the device (run_kmc's ``origin_metrics``): every metrics.csv gains the origin
columns, every run directory an origin_layers.csv (with ``--grains`` an origin_grains.csv), and gv_map.csv the columns
``Nucleated_grain_volume_frac`` and ``Nucleated_voxel_frac`` -- the share of the grain volume, and of the filled voxels, that
came from nucleation events -- from each run's last row (behind the solidification columns).  Without the flag the files are
what they were.
"""
import argparse
import os

import pandas as pd

from constants import ATOMIC_SPACING_W, DEFECT_PROB, N_SEEDS, RANDOM_SEED, T_MELT, VOXEL_SIZE
from kmc_simulation import beam_laser, run_gradient_boundary, run_kmc, run_kmc_ensemble


def check_args(L, n_steps, temps, nu_deps, seeds, ensemble, rng, run_kw, laser_powers=None, scan_speeds=None):
    """Driver arguments, checked before any device call."""
    if bool(laser_powers) != bool(scan_speeds):
        raise ValueError("--laser-power and --scan-speed come together (at least one value each)")
    if laser_powers and run_kw.get("mode", "A") != "A":
        raise ValueError("the laser axes need mode A (run_kmc refuses laser with mode B)")
    if rng not in ("reference", "counter"):
        raise ValueError("rng must be 'reference' or 'counter'")
    if int(seeds) < 1:
        raise ValueError("seeds must be >= 1")
    if ensemble:
        if run_kw:
            raise ValueError(f"--ensemble takes no run_kmc options ({sorted(run_kw)}): the RNG setting picks the mode")
        if not 1 <= L <= 128:
            raise ValueError("--ensemble covers 1 <= L <= 128")
    elif rng != "reference":
        raise ValueError("--rng counter needs --ensemble (the sequential equivalent is --mode B --box L)")
    if n_steps < 0 or not temps or not nu_deps:
        raise ValueError("need n_steps >= 0, at least one temperature and one nu_dep")


def gv_sweep(L=30, n_steps=2000, temps=(2800.0, 3100.0, 3400.0), nu_deps=(2e12, 2e13, 2e14), carbon=0.2,
             defect_fraction=DEFECT_PROB, n_seeds=N_SEEDS, out_dir="outputs/gv_sweep", seeds=1, ensemble=False, rng="reference",
             laser_powers=None, scan_speeds=None, laser_start=0.0, front=False, layers=False, texture=False,
             grains=False, solid=False, origin=False, remelt=False, thermal_substeps=1, thermal_scheme="explicit", hold_gradient=False,
             cooling_rate=0.0, scan=None, hatch=None, beam_depth=1, penetration=None, **run_kw):
    """``scan`` (a thermal_solver.scan_path pattern; with the laser axes and ``thermal_scheme="implicit"``): every point's laser
    follows that path with ``hatch`` voxels between tracks, absorbed over ``beam_depth`` planes (``penetration`` [m]: e-folding
    depth; None: uniform) -- run_kmc's laser option with a path, the source built on the device (``laser_start`` is not used).
    ``hold_gradient=True`` (with ``thermal_scheme="implicit"``): every run with run_kmc's ``thermal_boundary`` set to the
    boundary that holds its own initial ramp (``kmc_simulation.run_gradient_boundary``), lowered by ``cooling_rate`` [K/s];
    gv_map.csv gains ``CoolingRate_K_per_s`` behind ``G_over_V``.  An ensemble shares one boundary, so it needs one temperature.
    ``thermal_substeps`` (N or "stable"): every run with run_kmc's option of that name (mode "A"; one value for an ensemble).
    ``thermal_scheme`` ("explicit" or "implicit"): likewise.
    ``remelt`` (True or a threshold temperature): every run with run_kmc's ``remelt`` option (mode "A"; in an ensemble the
    shared ``remelt`` key of the configs).  ``run_kw`` goes to run_kmc unchanged -- e.g. ``mode="B", box=8`` runs every point of the map through the super-step
    engine (same metrics.csv columns; n_steps stays the number of executed events).  ``seeds=K`` runs every point with the
    seeds RANDOM_SEED .. RANDOM_SEED + K - 1; ``ensemble=True`` runs all runs of the map as one replica ensemble.
    ``laser_powers`` / ``scan_speeds`` (both or neither): two more axes, every point with run_kmc's ``laser`` option.
    ``front=True``: every run with ``front_metrics=True``; gv_map.csv gains the measured ``G_front_K_per_m``,
    ``V_front_m_per_s`` and ``G_over_V_front`` (inf when V is 0) of each run's last row behind the nominal columns.
    ``layers=True``: every run with ``layer_metrics=True``; gv_map.csv gains ``CET_height_um`` (-1.0: no transition) and
    ``InterceptRatio`` of each run's last row behind those.  ``texture=True``: every run with ``texture_metrics=True``;
    gv_map.csv gains ``GB_low_angle_frac`` and ``Pole_aligned_frac`` of each run's last row behind those.  ``grains=True``:
    every run with ``grain_metrics=True``; gv_map.csv gains ``Columnar_vol_frac`` and ``Grain_elong_mean`` of each run's last
    row behind those.  ``solid=True``: every run with ``solid_metrics=True``; gv_map.csv gains ``G_solid_K_per_m``,
    ``V_solid_m_per_s`` and ``G_over_V_solid`` (inf when V is 0) of each run's last row behind those.  ``origin=True``: every
    run with ``origin_metrics=True``; gv_map.csv gains ``Nucleated_grain_volume_frac`` and ``Nucleated_voxel_frac`` of each
    run's last row behind those."""
    check_args(L, n_steps, temps, nu_deps, seeds, ensemble, rng, run_kw, laser_powers, scan_speeds)
    if scan is None and (hatch is not None or beam_depth != 1 or penetration is not None):
        raise ValueError("--hatch, --beam-depth and --penetration describe a --scan")
    if scan is not None and not laser_powers:
        raise ValueError("--scan needs the laser axes (--laser-power and --scan-speed)")
    seeds = int(seeds)

    def laser_of(beam):
        if scan is not None:
            return beam_laser(beam[0], scan, beam[1], hatch, beam_depth, penetration)
        return dict(power=float(beam[0]), start=float(laser_start), speed=float(beam[1]))
    beams = [(p, v) for p in laser_powers for v in scan_speeds] if laser_powers else [None]
    runs = []
    for T_sub in temps:
        for nu_dep in nu_deps:
            for beam in beams:
                for s in range(seeds):
                    prefix = f"gv_sweep/T{int(T_sub)}_V{nu_dep:.0e}" + (f"_P{beam[0]:g}_S{beam[1]:g}" if beam else "") + \
                             f"_c_{int(carbon * 100)}" + (f"_seed{RANDOM_SEED + s}" if seeds > 1 else "")
                    runs.append((T_sub, nu_dep, RANDOM_SEED + s, prefix, beam))
    cfg = [dict(temp=T_sub, defect_fraction=defect_fraction, n_seeds=n_seeds, impurity_c=carbon, output_prefix=prefix,
                nu_dep=nu_dep, **({"seed": seed} if seeds > 1 else {}),
                **({"laser": laser_of(beam)} if beam else {}),
                **({"remelt": remelt} if remelt is not False and remelt is not None else {}))
           for T_sub, nu_dep, seed, prefix, beam in runs]
    opt = dict(**({"front_metrics": True} if front else {}), **({"layer_metrics": True} if layers else {}),
               **({"texture_metrics": True} if texture else {}), **({"grain_metrics": True} if grains else {}),
               **({"solid_metrics": True} if solid else {}), **({"origin_metrics": True} if origin else {}),
               **({"thermal_substeps": thermal_substeps} if thermal_substeps != 1 else {}),
               **({"thermal_scheme": thermal_scheme} if thermal_scheme != "explicit" else {}))
    if cooling_rate and not hold_gradient:
        raise ValueError("cooling_rate needs hold_gradient=True (it lowers the held faces)")
    if hold_gradient and ensemble and len(set(temps)) != 1:
        raise ValueError("hold_gradient with ensemble=True needs one temperature (the replicas share one boundary)")

    def held(T_sub):
        return {"thermal_boundary": run_gradient_boundary(L, T_sub, cooling_rate)} if hold_gradient else {}
    if ensemble:
        run_kmc_ensemble(cfg, L, n_steps, rng=rng, **opt, **held(temps[0]))
    else:
        for c in cfg:
            run_kmc(L=L, n_steps=n_steps, **c, **run_kw, **opt, **held(c["temp"]))
    rows = []
    for T_sub, nu_dep, seed, prefix, beam in runs:
        last = pd.read_csv(f"outputs/{prefix}/metrics.csv").iloc[-1]
        G = (T_MELT - T_sub) / (L * VOXEL_SIZE)                 # gradient of the initial ramp of this run
        V = nu_dep * ATOMIC_SPACING_W
        row = {"T_sub": T_sub, "nu_dep": nu_dep}
        if beam:
            row.update(power=beam[0], speed=beam[1])
        if seeds > 1:
            row["seed"] = seed
        row.update({"G_K_per_m": G, "V_m_per_s": V, "G_over_V": G / V,
                    **({"CoolingRate_K_per_s": float(cooling_rate)} if hold_gradient else {}),
                    "AspectRatio": last["AspectRatio"], "EquiaxedFraction": last["EquiaxedFraction"],
                    "GrainCount": last["GrainCount"], "NucleationCount": last["NucleationCount"],
                    "CET_Class": last["CET_Class"], "CET_Detected": last["CET_Detected"]})
        if front:
            Gf, Vf = float(last["G_front"]), float(last["V_front"])
            row.update({"G_front_K_per_m": Gf, "V_front_m_per_s": Vf, "G_over_V_front": Gf / Vf if Vf != 0.0 else float("inf")})
        if layers:
            row.update({"CET_height_um": float(last["CET_height_um"]), "InterceptRatio": float(last["InterceptRatio"])})
        if texture:
            row.update({"GB_low_angle_frac": float(last["GB_low_angle_frac"]), "Pole_aligned_frac": float(last["Pole_aligned_frac"])})
        if grains:
            row.update({"Columnar_vol_frac": float(last["Columnar_vol_frac"]), "Grain_elong_mean": float(last["Grain_elong_mean"])})
        if solid:
            Gs, Vs = float(last["G_solid"]), float(last["V_solid"])
            row.update({"G_solid_K_per_m": Gs, "V_solid_m_per_s": Vs, "G_over_V_solid": Gs / Vs if Vs != 0.0 else float("inf")})
        if origin:
            row.update({"Nucleated_grain_volume_frac": float(last["Nucleated_grain_volume_frac"]),
                        "Nucleated_voxel_frac": float(last["Nucleated_voxel_frac"])})
        rows.append(row)
    os.makedirs(out_dir, exist_ok=True)
    df = pd.DataFrame(rows)
    df.to_csv(os.path.join(out_dir, "gv_map.csv"), index=False)
    return df


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=30)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--temps", type=float, nargs="*", default=[2800.0, 3100.0, 3400.0])
    ap.add_argument("--nu-dep", type=float, nargs="*", default=[2e12, 2e13, 2e14])
    ap.add_argument("--carbon", type=float, default=0.2)
    ap.add_argument("--mode", choices=("A", "B"), default="A", help="A: exact loop (one event per sweep); B: super-steps")
    ap.add_argument("--box", type=int, default=8)
    ap.add_argument("--seeds", type=int, default=1, help="runs per point (seeds RANDOM_SEED ..); 1 = one run, no seed column")
    ap.add_argument("--ensemble", action="store_true", help="run the whole map as one replica ensemble")
    ap.add_argument("--rng", choices=("reference", "counter"), default="reference",
                    help="--ensemble: reference streams (= the sequential run's files) or counter uniforms (= --mode B --box L)")
    floats = lambda s: tuple(float(x) for x in s.split(",") if x)       # noqa: E731
    ap.add_argument("--laser-power", type=floats, default=None, help="P1,P2,... [W]: laser axis of the map (with --scan-speed)")
    ap.add_argument("--scan-speed", type=floats, default=None, help="V1,V2,... [voxels per temperature update]")
    ap.add_argument("--laser-start", type=float, default=0.0, help="beam centre at the first temperature update [voxels]")
    ap.add_argument("--scan", choices=("diagonal", "line", "raster", "serpentine"), default=None,
                    help="with the laser axes and --thermal-scheme implicit: the laser follows this scan path, its source built on "
                         "the device from a beam table (run_kmc laser with a path)")
    ap.add_argument("--hatch", type=float, default=None, metavar="H", help="--scan raster|serpentine: voxels between tracks")
    ap.add_argument("--beam-depth", type=int, default=1, metavar="D", help="--scan: planes from the top that absorb the beam")
    ap.add_argument("--penetration", type=float, default=None, metavar="M",
                    help="--beam-depth D > 1: e-folding depth of the absorption [m] (default: uniform over the D planes)")
    ap.add_argument("--front", action="store_true",
                    help="measure G and V at the growth front on the device: front columns in every metrics.csv and gv_map.csv")
    ap.add_argument("--layers", action="store_true",
                    help="layer-resolved grain structure on the device: layer columns in every metrics.csv, layers.csv, gv_map.csv")
    ap.add_argument("--texture", action="store_true",
                    help="boundary misorientation and pole histograms on the device: texture columns in every metrics.csv, "
                         "texture.csv, gv_map.csv")
    ap.add_argument("--grains", action="store_true",
                    help="per-grain table on the device: grain columns in every metrics.csv, grains.csv, gv_map.csv")
    ap.add_argument("--solid", action="store_true",
                    help="solidification map on the device: G and V at freezing in every metrics.csv, solid_layers.csv, gv_map.csv")
    ap.add_argument("--origin", action="store_true",
                    help="origin map on the device: origin columns in every metrics.csv, origin_layers.csv, gv_map.csv")
    ap.add_argument("--remelt", type=float, nargs="?", const=True, default=False, metavar="T",
                    help="remelting on the device in every run: occupied voxels at or above T (default T_MELT) become empty "
                         "behind every temperature update (run_kmc remelt)")
    ap.add_argument("--thermal-substeps", type=lambda s: s if s == "stable" else int(s), default=1, metavar="N|stable",
                    help="every temperature update as N explicit steps of dt / N on the device ('stable': the smallest stable N, 17; "
                         "run_kmc thermal_substeps, mode A)")
    ap.add_argument("--thermal-scheme", choices=("explicit", "implicit"), default="explicit",
                    help="every temperature update as locally one-dimensional backward-Euler steps on the device, stable at any dt "
                         "(run_kmc thermal_scheme, mode A)")
    ap.add_argument("--hold-gradient", action="store_true",
                    help="with --thermal-scheme implicit: fixed faces at the next values of each run's initial ramp, so the imposed G "
                         "lasts through the run (run_kmc thermal_boundary)")
    ap.add_argument("--cooling-rate", type=float, default=0.0, metavar="K_PER_S",
                    help="--hold-gradient: the held faces fall by this rate; recorded beside G and V in gv_map.csv")
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
    print(gv_sweep(a.L, a.steps, tuple(a.temps), tuple(a.nu_dep), a.carbon, seeds=a.seeds, ensemble=a.ensemble, rng=a.rng,
                   laser_powers=a.laser_power, scan_speeds=a.scan_speed, laser_start=a.laser_start, front=a.front,
                   layers=a.layers, texture=a.texture, grains=a.grains, solid=a.solid, origin=a.origin, remelt=a.remelt,
                   thermal_substeps=a.thermal_substeps, thermal_scheme=a.thermal_scheme, hold_gradient=a.hold_gradient,
                   cooling_rate=a.cooling_rate, scan=a.scan, hatch=a.hatch, beam_depth=a.beam_depth, penetration=a.penetration,
                   **kw).to_string(index=False))
