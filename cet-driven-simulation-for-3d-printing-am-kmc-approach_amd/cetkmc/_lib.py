"""Loader + ctypes prototypes for include/cetkmc.h."""
import ctypes as C
import glob
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include")
SO_PATH = os.path.join(CSRC, "libcetkmc_hip.so")


def sources():
    """Every file the library is compiled from: csrc/*.hip, csrc/*.hpp, include/*.h (globbed, so that a new header
    cannot be forgotten by the staleness check)."""
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")) +
                  glob.glob(os.path.join(INCLUDE, "*.h")))


HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
               "-fno-fast-math", "-I/opt/rocm/include"]


class Params(C.Structure):
    _fields_ = [
        ("nu", C.c_double), ("nu_dep", C.c_double), ("E_b", C.c_double * 3), ("E_diff", C.c_double * 3),
        ("kT", C.c_double), ("T_melt", C.c_double), ("I0", C.c_double), ("delta_T_c", C.c_double),
        ("K_nuc", C.c_double), ("beta_imp_nuc", C.c_double), ("max_imp_frac", C.c_double),
        ("rate_threshold", C.c_double), ("anisotropy", C.c_double), ("impurity_re", C.c_double),
        ("impurity_c", C.c_double),
        ("alpha", C.c_double), ("inv_dx2", C.c_double), ("T_clip_lo", C.c_double), ("T_clip_hi", C.c_double),
        ("T_nan", C.c_double), ("rho_cp", C.c_double), ("latent_coef", C.c_double),
    ]


class Event(C.Structure):
    _fields_ = [("type", C.c_int32), ("pos", C.c_int32 * 3), ("target", C.c_int32 * 3), ("atom", C.c_int32),
                ("rate", C.c_double), ("dep_rank", C.c_int64), ("theta", C.c_double), ("phi", C.c_double)]


class SweepInfo(C.Structure):
    _fields_ = [("total", C.c_double), ("n_events", C.c_int64), ("n_dep", C.c_int64)]


class RunArgs(C.Structure):
    _fields_ = [
        ("step0", C.c_int64), ("n_steps", C.c_int64), ("defect_fraction", C.c_double),
        ("u_pick", C.POINTER(C.c_double)), ("u_defect", C.POINTER(C.c_double)), ("u_np", C.POINTER(C.c_double)),
        ("np_cap", C.c_int64), ("rng_mode", C.c_int32), ("seed", C.c_uint64), ("thermal_mode", C.c_int32),
        ("thermal_dt", C.c_double), ("q_planes", C.POINTER(C.c_double)), ("n_q", C.c_int64),
        ("use_latent", C.c_int32), ("profile", C.c_int32), ("incremental", C.c_int32),
    ]


class SuperArgs(C.Structure):
    _fields_ = [
        ("step0", C.c_int64), ("n_steps", C.c_int64), ("box", C.c_int32), ("defect_fraction", C.c_double),
        ("seed", C.c_uint64), ("thermal_mode", C.c_int32), ("thermal_dt", C.c_double),
        ("q_planes", C.POINTER(C.c_double)), ("n_q", C.c_int64), ("use_latent", C.c_int32), ("null_events", C.c_int32),
    ]


class LocalArgs(C.Structure):
    _fields_ = [
        ("step0", C.c_int64), ("n_steps", C.c_int64), ("box", C.c_int32), ("defect_fraction", C.c_double),
        ("seed", C.c_uint64), ("thermal_mode", C.c_int32), ("thermal_dt", C.c_double), ("max_events", C.c_int32),
        ("horizon_events", C.c_double),
    ]


class LaneTableInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("fresh", "chunks", "usable", "poisoned", "builds", "builds_thermal")]


class Counters(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("steps", "sweeps", "incremental_steps", "thermal_updates", "supersteps", "bytes_h2d",
                                         "bytes_d2h", "alg_bytes_sweep", "alg_bytes_thermal", "profiled_steps")] + \
               [(n, C.c_double) for n in ("ms_thermal", "ms_interface", "ms_sweep", "ms_dirty_rows", "ms_reduce", "ms_select_apply")] + \
               [(n, C.c_int64) for n in ("alg_bytes_table", "table_updates", "interface_launches")] + \
               [("ms_comm", C.c_double), ("comm_calls", C.c_int64), ("deferred_steps", C.c_int64),
                ("early_tiles", C.c_int64)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64)


class HostComm(C.Structure):
    _fields_ = [("allgather", ALLGATHER_FN), ("exchange", EXCHANGE_FN), ("user", C.c_void_p)]


class RunResult(C.Structure):
    _fields_ = [
        ("steps_done", C.c_int64), ("status", C.c_int32), ("np_used", C.c_int64), ("q_used", C.c_int64),
        ("nucleation_count", C.c_int64), ("sweep_ms_total", C.c_double), ("sweep_launches", C.c_int64),
        ("wall_ms", C.c_double), ("full_sweeps", C.c_int64), ("min_margin", C.c_double),
    ]


class EnsArgs(C.Structure):
    _fields_ = [
        ("step0", C.c_int64), ("n_steps", C.c_int64), ("defect_fraction", C.POINTER(C.c_double)),
        ("u_pick", C.POINTER(C.c_double)), ("u_defect", C.POINTER(C.c_double)), ("u_np", C.POINTER(C.c_double)),
        ("np_stride", C.c_int64), ("seed", C.POINTER(C.c_uint64)), ("rng_mode", C.c_int32), ("thermal_mode", C.c_int32),
        ("thermal_dt", C.c_double), ("q_planes", C.POINTER(C.c_double)), ("n_q", C.c_int64), ("n_sets", C.c_int32),
        ("q_set", C.POINTER(C.c_int32)), ("use_latent", C.c_int32),
    ]


class EnsAnalysis(C.Structure):
    _fields_ = [
        ("threshold", C.c_double), ("species", C.c_int32), ("pad", C.c_int32), ("n_clusters", C.POINTER(C.c_int64)),
        ("species_counts", C.POINTER(C.c_int64)), ("nucleation_count", C.POINTER(C.c_int64)), ("n_gathered", C.POINTER(C.c_int64)),
    ]


class FrontStats(C.Structure):
    _fields_ = [
        ("n_front", C.c_int64), ("n_skipped", C.c_int64), ("pos_sum", C.c_int64 * 3), ("G_sum", C.c_double),
        ("G_min", C.c_double), ("G_max", C.c_double), ("Gi_sum", C.c_double), ("T_sum", C.c_double), ("n_melt", C.c_int64),
        ("melt_bbox", C.c_int32 * 6),
    ]


class LayerRec(C.Structure):
    _fields_ = [
        ("n_occ", C.c_int64), ("n_start", C.c_int64), ("n_eq", C.c_int64), ("seg", C.c_int64 * 3), ("cut", C.c_int64 * 3),
        ("occ_state", C.c_int64 * 4), ("gb_state", C.c_int64 * 4), ("pad", C.c_int64),
    ]


class GrainRec(C.Structure):
    _fields_ = [
        ("n", C.c_int64), ("sum", C.c_int64 * 3), ("sq", C.c_int64 * 6), ("n_state", C.c_int64 * 4), ("nb", C.c_int64 * 4),
        ("first_theta", C.c_double), ("first_phi", C.c_double),
    ]


class TextureArgs(C.Structure):
    _fields_ = [
        ("n_bins", C.c_int32), ("pad", C.c_int32), ("gb_edges", C.POINTER(C.c_double)), ("pole_edges", C.POINTER(C.c_double)),
        ("axis", C.c_double * 3),
    ]


class SolidInfo(C.Structure):
    _fields_ = [("n_new", C.c_int64), ("n_cleared", C.c_int64), ("n_recorded", C.c_int64)]


class SolidArgs(C.Structure):
    _fields_ = [("qscale", C.c_double * 4)]


class SolidRec(C.Structure):
    _fields_ = [("n_rec", C.c_int64), ("n_bad", C.c_int64), ("n_cooling", C.c_int64), ("stamp_sum", C.c_int64),
                ("stamp_min", C.c_int64), ("stamp_max", C.c_int64), ("q", C.c_int64 * 4)]


class OriginRec(C.Structure):
    _fields_ = [("n_occ", C.c_int64), ("n_by", C.c_int64 * 4), ("n_unrec", C.c_int64), ("n_left", C.c_int64),
                ("ord_sum", C.c_int64), ("ord_min", C.c_int64), ("ord_max", C.c_int64), ("birth", C.c_int64), ("pad", C.c_int64)]


class RemeltInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("passes", "n_melted", "n_melted_last", "n_appended")]


class SubstepInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("updates", "substeps", "launches", "blocked_launches")]


class ImplicitInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("updates", "steps", "launches", "coeff_uploads")]


class ThermalBoundary(C.Structure):
    _fields_ = [(n, C.c_double * 6) for n in ("beta", "T_ext", "ramp")]


class BoundaryInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("updates", "steps", "launches", "coeff_uploads")]


class Beam(C.Structure):
    _fields_ = [("u0", C.c_int64), ("n_u", C.c_int32), ("depth", C.c_int32), ("amp", C.POINTER(C.c_double)),
                ("gj", C.POINTER(C.c_double)), ("gk", C.POINTER(C.c_double)), ("fi", C.POINTER(C.c_double))]


class BeamInfo(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("updates", "steps", "launches", "table_uploads")]


class Shift(C.Structure):
    _fields_ = [("d", C.c_int32 * 3), ("fill_state", C.c_int32), ("T_mode", C.c_int32), ("pad", C.c_int32),
                ("fill_T", C.c_double), ("fill_theta", C.c_double), ("fill_phi", C.c_double)]


class ShiftInfo(C.Structure):
    _fields_ = [("calls", C.c_int64), ("kept", C.c_int64), ("exposed", C.c_int64), ("dropped", C.c_int64 * 6)]


STRUCT_MIRRORS = {"params": Params, "event": Event, "sweep_info": SweepInfo, "run_args": RunArgs, "run_result": RunResult,
                  "super_args": SuperArgs, "counters": Counters, "host_comm": HostComm, "ens_args": EnsArgs,
                  "ens_analysis": EnsAnalysis, "front_stats": FrontStats, "layer_rec": LayerRec,
                  "texture_args": TextureArgs, "grain_rec": GrainRec, "solid_info": SolidInfo, "solid_args": SolidArgs,
                  "solid_rec": SolidRec, "origin_rec": OriginRec, "local_args": LocalArgs,
                  "remelt_info": RemeltInfo, "substep_info": SubstepInfo, "implicit_info": ImplicitInfo,
                  "thermal_boundary": ThermalBoundary, "boundary_info": BoundaryInfo,
                  "beam": Beam, "beam_info": BeamInfo, "shift": Shift, "shift_info": ShiftInfo}

# name -> (restype, argtypes); every symbol include/cetkmc.h declares
_P = C.POINTER
PROTOTYPES = {
    "cetkmc_last_error": (C.c_char_p, []),
    "cetkmc_abi_version": (C.c_int, []),
    "cetkmc_source_hash": (C.c_char_p, []),
    "cetkmc_struct_size": (C.c_int, [C.c_char_p]),
    "cetkmc_dirty_offset": (C.c_int, [C.c_int, C.c_int]),
    "cetkmc_stale_row": (C.c_int, [C.c_int, _P(C.c_int), _P(C.c_int), C.c_int, C.c_int]),
    "cetkmc_stale_rows": (C.c_int, [C.c_int, _P(C.c_int), _P(C.c_int), C.c_int, C.c_void_p]),
    "cetkmc_table_tile_of": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "cetkmc_early_tile_row": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "cetkmc_lane_needs_values": (C.c_int, [C.c_uint64]),
    "cetkmc_lane_request": (C.c_int, [C.c_uint64, C.c_int]),
    "cetkmc_lane_table": (C.c_int, [C.c_void_p, _P(LaneTableInfo)]),
    "cetkmc_lane_table_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "cetkmc_lane_quad_node": (None, [_P(C.c_double), C.c_int, _P(C.c_double), _P(C.c_int)]),
    "cetkmc_tree8": (C.c_double, [_P(C.c_double)]),
    "cetkmc_invalidates": (C.c_int, [C.c_char_p]),
    "cetkmc_device_count": (C.c_int, [_P(C.c_int)]),
    "cetkmc_create": (C.c_int, [_P(Params), C.c_int, C.c_int, _P(C.c_int), _P(C.c_void_p)]),
    "cetkmc_get_unique_id": (C.c_int, [C.c_char_p]),
    "cetkmc_create_rank": (C.c_int, [_P(Params), C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _P(C.c_void_p)]),
    "cetkmc_create_rank_host": (C.c_int, [_P(Params), C.c_int, C.c_int, C.c_int, C.c_int, _P(HostComm), _P(C.c_void_p)]),
    "cetkmc_destroy": (C.c_int, [C.c_void_p]),
    "cetkmc_set_params": (C.c_int, [C.c_void_p, _P(Params)]),
    "cetkmc_sync": (C.c_int, [C.c_void_p]),
    "cetkmc_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "cetkmc_owned_planes": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_int)]),
    "cetkmc_upload": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_upload_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_download_planes": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_set_defects": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_set_prev_state": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_thermal_cet": (C.c_int, [C.c_void_p, C.c_double, C.c_int]),
    "cetkmc_thermal_laser": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int]),
    "cetkmc_rate_sweep": (C.c_int, [C.c_void_p, _P(SweepInfo)]),
    "cetkmc_select": (C.c_int, [C.c_void_p, C.c_double, _P(Event)]),
    "cetkmc_apply": (C.c_int, [C.c_void_p, _P(Event), C.c_double, C.c_double, C.c_int]),
    "cetkmc_enumerate_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    "cetkmc_row_sums": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_run_steps": (C.c_int, [C.c_void_p, _P(RunArgs), _P(RunResult), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_stage_inputs": (C.c_int, [C.c_void_p, _P(RunArgs)]),
    "cetkmc_run_supersteps": (C.c_int, [C.c_void_p, _P(SuperArgs), _P(RunResult), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_run_supersteps_local": (C.c_int, [C.c_void_p, _P(LocalArgs), _P(RunResult), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "cetkmc_get_counters": (C.c_int, [C.c_void_p, _P(Counters), C.c_int]),
    "cetkmc_cluster": (C.c_int, [C.c_void_p, C.c_double, _P(C.c_int64)]),
    "cetkmc_cluster_stats": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_cluster_labels": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_species_counts": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_gather_species": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, _P(C.c_int64)]),
    "cetkmc_set_defects_sparse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "cetkmc_nucleation_count": (C.c_int64, [C.c_void_p]),
    "cetkmc_reset_counters": (C.c_int, [C.c_void_p]),
    "cetkmc_time_sweeps": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_double)]),
    "cetkmc_event_overhead": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_double)]),
    "cetkmc_comm_selftest": (C.c_int, [C.c_void_p, C.c_int64, _P(C.c_double)]),
    "cetkmc_create_ensemble": (C.c_int, [_P(Params), C.c_int, C.c_int, C.c_int, _P(C.c_void_p)]),
    "cetkmc_ensemble_replica": (C.c_int, [C.c_void_p, C.c_int, _P(C.c_void_p)]),
    "cetkmc_run_ensemble": (C.c_int, [C.c_void_p, _P(EnsArgs), _P(RunResult), C.c_void_p, C.c_void_p]),
    "cetkmc_ensemble_analyze": (C.c_int, [C.c_void_p, _P(EnsAnalysis)]),
    "cetkmc_ensemble_analysis_data": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_ensemble_set_defects_sparse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_front_stats": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "cetkmc_ensemble_front_stats": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "cetkmc_layer_profile": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "cetkmc_ensemble_layer_profile": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "cetkmc_cluster_import": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_int64)]),
    "cetkmc_ensemble_cluster_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_texture_profile": (C.c_int, [C.c_void_p, _P(TextureArgs), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_ensemble_texture_profile": (C.c_int, [C.c_void_p, _P(TextureArgs), C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_grain_table": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "cetkmc_ensemble_grain_table": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_solid_begin": (C.c_int, [C.c_void_p]),
    "cetkmc_solid_end": (C.c_int, [C.c_void_p]),
    "cetkmc_solid_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p]),
    "cetkmc_solid_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_solid_profile": (C.c_int, [C.c_void_p, _P(SolidArgs), C.c_void_p, C.c_int64, C.c_void_p]),
    "cetkmc_ensemble_solid_begin": (C.c_int, [C.c_void_p]),
    "cetkmc_ensemble_solid_end": (C.c_int, [C.c_void_p]),
    "cetkmc_ensemble_solid_update": (C.c_int, [C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_void_p]),
    "cetkmc_ensemble_solid_profile": (C.c_int, [C.c_void_p, _P(SolidArgs), C.c_void_p, C.c_void_p]),
    "cetkmc_origin_begin": (C.c_int, [C.c_void_p]),
    "cetkmc_origin_end": (C.c_int, [C.c_void_p]),
    "cetkmc_origin_absorb_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "cetkmc_origin_read": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_origin_census": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_origin_seq": (C.c_int64, [C.c_void_p]),
    "cetkmc_origin_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "cetkmc_ensemble_origin_begin": (C.c_int, [C.c_void_p]),
    "cetkmc_ensemble_origin_end": (C.c_int, [C.c_void_p]),
    "cetkmc_ensemble_origin_census": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_ensemble_origin_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cetkmc_set_remelt": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "cetkmc_remelt": (C.c_int, [C.c_void_p, C.c_double, _P(RemeltInfo)]),
    "cetkmc_time_remelt": (C.c_int, [C.c_void_p, C.c_double, C.c_int, _P(C.c_double)]),
    "cetkmc_get_remelt_info": (C.c_int, [C.c_void_p, _P(RemeltInfo)]),
    "cetkmc_ensemble_set_remelt": (C.c_int, [C.c_void_p, C.c_int, C.c_double]),
    "cetkmc_ensemble_remelt_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cetkmc_set_thermal_substeps": (C.c_int, [C.c_void_p, C.c_int]),
    "cetkmc_ensemble_set_thermal_substeps": (C.c_int, [C.c_void_p, C.c_int]),
    "cetkmc_get_substep_info": (C.c_int, [C.c_void_p, _P(SubstepInfo)]),
    "cetkmc_time_thermal": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _P(C.c_double)]),
    "cetkmc_set_thermal_scheme": (C.c_int, [C.c_void_p, C.c_int]),
    "cetkmc_ensemble_set_thermal_scheme": (C.c_int, [C.c_void_p, C.c_int]),
    "cetkmc_get_implicit_info": (C.c_int, [C.c_void_p, _P(ImplicitInfo)]),
    "cetkmc_implicit_coeffs": (C.c_int, [C.c_int, C.c_double, _P(C.c_double), _P(C.c_double)]),
    "cetkmc_set_thermal_boundary": (C.c_int, [C.c_void_p, _P(ThermalBoundary)]),
    "cetkmc_ensemble_set_thermal_boundary": (C.c_int, [C.c_void_p, _P(ThermalBoundary)]),
    "cetkmc_get_thermal_boundary": (C.c_int, [C.c_void_p, _P(ThermalBoundary), _P(BoundaryInfo)]),
    "cetkmc_set_beam": (C.c_int, [C.c_void_p, _P(Beam)]),
    "cetkmc_ensemble_set_beam": (C.c_int, [C.c_void_p, C.c_int, _P(Beam), _P(C.c_int32)]),
    "cetkmc_get_beam_info": (C.c_int, [C.c_void_p, _P(BeamInfo)]),
    "cetkmc_thermal_beam": (C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int, C.c_int]),
    "cetkmc_shift": (C.c_int, [C.c_void_p, _P(Shift), _P(ShiftInfo)]),
    "cetkmc_ensemble_shift": (C.c_int, [C.c_void_p, _P(Shift), _P(ShiftInfo)]),
    "cetkmc_time_shift": (C.c_int, [C.c_void_p, _P(Shift), _P(ShiftInfo), _P(C.c_double)]),
    "cetkmc_implicit_coeffs_bc": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_double, _P(C.c_double), _P(C.c_double)]),
}


LAST_BUILD = None      # "compiled" | "reused" after build_library()


def source_hash():
    """sha256 (16 hex digits) over every source of the library, in name order: what the library reports through
    cetkmc_source_hash() when it was compiled from exactly these files."""
    import hashlib
    h = hashlib.sha256()
    for f in sources():
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def library_hash(so_path=None):
    """the source hash compiled into an existing library, or None (missing file / library from before the hash).  Read from
    the file's bytes (marker "cetkmc-source-hash="), NOT by loading it: a library loaded once stays the one the process
    sees under that path, also after build_library() has replaced the file."""
    so_path = so_path or SO_PATH
    if not os.path.exists(so_path):
        return None
    marker = b"cetkmc-source-hash="
    with open(so_path, "rb") as f:
        data = f.read()
    at = data.find(marker)
    if at < 0:
        return None
    end = data.find(b"\0", at)
    return data[at + len(marker):end].decode(errors="replace")


def build_library(force=False, verbose=False):
    """hipcc cross-compiles for gfx950 without a GPU; the .so stays in-tree (csrc/).  Recompiles when the library is missing
    or was compiled from other sources than the ones beside it (source hash compiled in; file times are not trusted: a
    checkout or a copy changes them)."""
    global LAST_BUILD
    want = source_hash()
    if not force and library_hash() == want:
        LAST_BUILD = "reused"
        return SO_PATH
    import fcntl
    # several processes may import at once (torchrun ranks, the multi-process tests): one compiles, the others wait for the
    # lock and then find the finished library; hipcc writes a temporary file that is renamed into place, so a concurrent
    # dlopen never sees a half-written library
    with open(SO_PATH + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and library_hash() == want:
                LAST_BUILD = "reused"
                return SO_PATH
            LAST_BUILD = "compiled"
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            tmp = f"{SO_PATH}.tmp.{os.getpid()}"
            cmd = [hipcc] + HIPCC_FLAGS + [f'-DCETKMC_SRC_HASH="{want}"', os.path.join(CSRC, "cetkmc_hip.hip"), "-o", tmp, "-ldl"]
            if verbose:
                print(" ".join(cmd))
            try:
                subprocess.check_call(cmd, cwd=CSRC)
                os.replace(tmp, SO_PATH)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return SO_PATH


_lib = None


def load():
    """Load libcetkmc_hip.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    so_path = os.environ.get("CETKMC_LIB", SO_PATH)       # alternative build of the same library (A/B timing only)
    if "CETKMC_LIB" not in os.environ and os.path.exists(so_path) and library_hash(so_path) != source_hash() \
            and os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        build_library()        # a library compiled from other sources than the ones beside it: recompile (hipcc is here)
    if not os.path.exists(so_path):
        raise RuntimeError(
            f"{so_path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  cetkmc has no CPU fallback.")
    lib = C.CDLL(so_path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.cetkmc_abi_version() != 1:
        raise RuntimeError("libcetkmc_hip.so ABI version mismatch")
    if "CETKMC_LIB" not in os.environ:        # (an explicitly chosen alternative build is the caller's business)
        have, want = lib.cetkmc_source_hash().decode(), source_hash()
        if have != want:
            raise RuntimeError(f"{so_path} was compiled from other sources (hash {have}, sources {want}): rebuild it with "
                               "`python -c 'import __graft_entry__ as g; g.build()'`")
    for name, mirror in STRUCT_MIRRORS.items():
        if lib.cetkmc_struct_size(name.encode()) != C.sizeof(mirror):
            raise RuntimeError(f"libcetkmc_hip.so: struct {name} is {lib.cetkmc_struct_size(name.encode())} bytes, "
                               f"the Python mirror {C.sizeof(mirror)} (stale build?)")
    _lib = lib
    return lib
