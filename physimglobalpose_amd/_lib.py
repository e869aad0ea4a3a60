"""ctypes binding of libpgp.so (include/pgp.h).  Fails loudly when the HIP library is missing:
there is no Python, torch or CPU fallback for any entry point."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# PGP_LIB: a diagnostic / A-B build of the same library (tools/ab/*.so), never a different implementation
LIB_PATH = os.environ.get("PGP_LIB") or os.path.join(HERE, "libpgp.so")

PGP_MODE_PLAIN = 0
PGP_MODE_WEIGHTED = 1

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int)


class IndexInfo(C.Structure):
    _fields_ = [("n_scene", C.c_int), ("n_model", C.c_int),
                ("grid_nx", C.c_int), ("grid_ny", C.c_int), ("grid_nz", C.c_int),
                ("cell_size", C.c_float), ("delta", C.c_float),
                ("n_cells", C.c_longlong), ("n_candidates", C.c_longlong),
                ("n_occupied", C.c_longlong), ("bytes_index", C.c_longlong), ("build_ms", C.c_float),
                ("sparse", C.c_int), ("n_blocks", C.c_longlong)]


class IcpParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("trim_fraction", C.c_float),
                ("max_corr_dist", C.c_float), ("energy_ratio", C.c_float)]


class IcpOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int), ("trim_fraction", C.c_float), ("max_corr_dist", C.c_float),
                ("energy_ratio", C.c_float), ("error_metric", C.c_int), ("transformation_epsilon", C.c_float),
                ("relative_mse", C.c_float), ("absolute_mse", C.c_float), ("min_diff_rot", C.c_float),
                ("min_diff_trans", C.c_float), ("smooth_length", C.c_int), ("nn_search", C.c_int)]


class IcpJob(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("d_src4", C.c_void_p), ("n_src", C.c_int), ("d_tgt4", C.c_void_p), ("n_tgt", C.c_int),
                ("d_T", C.c_void_p), ("n", C.c_int), ("d_energy", C.c_void_p), ("d_iters", C.c_void_p)]


class MultiIcpJob(C.Structure):
    _fields_ = [("src_xyz", C.POINTER(C.c_float)), ("n_src", C.c_int), ("tgt_xyz", C.POINTER(C.c_float)), ("n_tgt", C.c_int),
                ("T", C.POINTER(C.c_float)), ("n", C.c_int), ("energy", C.POINTER(C.c_float)), ("iters", C.POINTER(C.c_int))]


class MultiInfo(C.Structure):
    _fields_ = [("n_local", C.c_int), ("world", C.c_int), ("rank0", C.c_int), ("rccl_ranks", C.c_int), ("emulated", C.c_int),
                ("devices", C.c_int * 16), ("exchanges", C.c_longlong)]


class Camera(C.Structure):
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("z_near", C.c_float), ("z_max", C.c_float)]


class ClusterParams(C.Structure):
    _fields_ = [("accept_fraction", C.c_float), ("rot_thresh_deg", C.c_float), ("trans_thresh", C.c_float)]


class SegmentOptions(C.Structure):
    _fields_ = [("z_min", C.c_double), ("z_max", C.c_double), ("voxel_leaf", C.c_float), ("mls_radius", C.c_float),
                ("filter_radius", C.c_float), ("min_neighbors", C.c_int), ("min_points", C.c_int), ("delta", C.c_float)]


PGP_PLANE_STOP_ADAPTIVE = 0
PGP_PLANE_STOP_ALL = 1


class PlaneOptions(C.Structure):
    _fields_ = [("threshold", C.c_float), ("max_iterations", C.c_int), ("probability", C.c_double), ("stop", C.c_int),
                ("optimize", C.c_int), ("seed", C.c_ulonglong)]


class PlaneInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("chosen", C.c_int), ("n_evaluated", C.c_int), ("n_valid", C.c_int),
                ("n_candidates", C.c_int), ("sampled_inliers", C.c_int), ("penalty", C.c_double),
                ("sampled", C.c_float * 4)]


class ComponentsOptions(C.Structure):
    _fields_ = [("z_min", C.c_double), ("z_max", C.c_double), ("tolerance", C.c_float), ("connectivity", C.c_int),
                ("min_pixels", C.c_int), ("max_pixels", C.c_int)]


class CreaseOptions(C.Structure):
    _fields_ = [("normal_step", C.c_int), ("smooth_radius", C.c_int), ("crease_step", C.c_int), ("concavity", C.c_float),
                ("grow_passes", C.c_int)]


class ComponentInfo(C.Structure):
    _fields_ = [("root", C.c_int), ("pixels", C.c_int), ("u_min", C.c_int), ("u_max", C.c_int), ("v_min", C.c_int),
                ("v_max", C.c_int), ("z_min", C.c_float), ("z_max", C.c_float), ("sum_um", C.c_longlong * 3)]


class PpfOptions(C.Structure):
    _fields_ = [("ref_step", C.c_int), ("n_bins", C.c_int), ("peaks_per_ref", C.c_int), ("min_vote_fraction", C.c_float),
                ("min_votes", C.c_int)]


class V4pcsOptions(C.Structure):
    _fields_ = [("seed", C.c_ulonglong), ("n_bases", C.c_int), ("max_attempts", C.c_int), ("triangle_trials", C.c_int),
                ("fourth_trials", C.c_int), ("max_base_diameter", C.c_float), ("eps", C.c_float), ("max_per_base", C.c_int),
                ("per_base_cap", C.c_int)]


class Super4pcsOptions(C.Structure):
    _fields_ = [("seed", C.c_ulonglong), ("n_bases", C.c_int), ("max_attempts", C.c_int), ("triangle_trials", C.c_int),
                ("max_base_diameter", C.c_float), ("eps", C.c_float), ("max_per_base", C.c_int)]


class PairGates(C.Structure):
    _fields_ = [("max_normal_difference", C.c_float), ("max_color_distance", C.c_float), ("max_translation_distance", C.c_float),
                ("max_angle", C.c_float), ("directed", C.c_int)]


class PhysicsOptions(C.Structure):
    _fields_ = [("dt", C.c_float), ("steps", C.c_int), ("gravity", C.c_float * 3), ("linear_damping", C.c_float),
                ("angular_damping", C.c_float), ("friction", C.c_float), ("iterations", C.c_int), ("erp", C.c_float)]


class PhysicsInfo(C.Structure):
    _fields_ = [("n_contacts", C.c_int), ("min_depth", C.c_float), ("lin_speed", C.c_float), ("ang_speed", C.c_float)]


class TricpOptions(C.Structure):
    _fields_ = [("trim_fraction", C.c_float), ("removal_radius", C.c_float), ("energy_ratio", C.c_float),
                ("max_iterations", C.c_int)]


class TricpObject(C.Structure):
    _fields_ = [("model_xyz", C.POINTER(C.c_float)), ("n_model", C.c_int), ("segment_xyz", C.POINTER(C.c_float)),
                ("n_segment", C.c_int)]


PGP_TRICP_MAX_SEGMENT = 4096
PGP_TRICP_MAX_STATICS = 16
PGP_TRICP_MAX_MODEL = 65535

PGP_MCTS_ROLLOUT_RANDOM = 0
PGP_MCTS_ROLLOUT_LCP = 1
PGP_MCTS_MAX_OBJECTS = 17
PGP_MCTS_STOP_EXPANSIONS, PGP_MCTS_STOP_ITERATIONS, PGP_MCTS_STOP_EXHAUSTED, PGP_MCTS_STOP_TIME = 1, 2, 3, 4


def mcts_types():
    """The MCTS structures of include/pgp.h (pgp_mcts_options, _object, _info, _record), built on first use: the entry
    points take them as void pointers here."""
    global _mcts_types
    if _mcts_types is None:
        class MctsOptions(C.Structure):
            _fields_ = [("max_expansions", C.c_longlong), ("max_iterations", C.c_int), ("max_seconds", C.c_float),
                        ("alpha", C.c_float), ("explanation_threshold", C.c_float), ("rollout", C.c_int),
                        ("seed", C.c_ulonglong), ("leaves_per_step", C.c_int), ("virtual_cost", C.c_float),
                        ("physics", PhysicsOptions)]

        class MctsObject(C.Structure):
            _fields_ = [("shape_id", C.c_int), ("vertices", C.POINTER(C.c_float)), ("vertex_stride", C.c_int),
                        ("n_vert", C.c_int), ("triangles", C.POINTER(C.c_int)), ("n_tri", C.c_int), ("n_hyp", C.c_int),
                        ("T", C.POINTER(C.c_float)), ("scores", C.POINTER(C.c_float))]

        class MctsInfo(C.Structure):
            _fields_ = [("descents", C.c_longlong), ("steps", C.c_longlong), ("expansions", C.c_longlong),
                        ("settle_evaluations", C.c_longlong), ("stop_reason", C.c_int), ("elapsed_ms", C.c_float)]

        class MctsRecord(C.Structure):
            _fields_ = [("step", C.c_int), ("t", C.c_int), ("depth", C.c_int), ("hyp", C.c_int * PGP_MCTS_MAX_OBJECTS),
                        ("evaluated", C.c_int), ("render_score", C.c_float), ("reward", C.c_float)]

        _mcts_types = (MctsOptions, MctsObject, MctsInfo, MctsRecord)
    return _mcts_types


_mcts_types = None


# every symbol include/pgp.h declares: (restype, argtypes)
SIGNATURES = {
    "pgp_version": (C.c_int, []),
    "pgp_last_error": (C.c_char_p, []),
    "pgp_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "pgp_destroy": (C.c_int, [C.c_void_p]),
    "pgp_center": (C.c_int, [_f, C.c_int, _f, C.c_int, _f, C.c_int, _f, _f]),
    "pgp_weights_from_image": (C.c_int, [_f, C.c_int, _f, _f, C.POINTER(C.c_ushort), C.c_int, C.c_int, _f]),
    "pgp_image_rows_needed": (C.c_int, [_f, C.c_int, _f, _f, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "pgp_set_scene": (C.c_int, [C.c_void_p, _f, _f, _f, C.c_int, C.c_float]),
    "pgp_set_model": (C.c_int, [C.c_void_p, _f, _f, C.c_int]),
    "pgp_score_lcp": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_int, C.c_float, _f, _i, _i, _f]),
    "pgp_reserve": (C.c_int, [C.c_void_p, C.c_int]),
    "pgp_score_lcp_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_settle_best_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_registered": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_float, _i, _i]),
    "pgp_registered_model": (C.c_int, [C.c_void_p, _f, _f, _f, C.c_int, C.c_float, _i, _i]),
    "pgp_find_congruent_4pcs": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float, _i, C.c_int, _i, C.c_int,
                                          _i, C.c_int, _i]),
    "pgp_running_best": (C.c_int, [_f, C.c_int, _i, _i]),
    "pgp_set_search_model": (C.c_int, [C.c_void_p, _f, C.c_int]),
    "pgp_set_ppf_map": (C.c_int, [C.c_void_p, _i, _i, _i, C.c_int]),
    "pgp_set_ppf_map_from_model": (C.c_int, [C.c_void_p, _f, _f, C.c_int, _i, C.POINTER(C.c_longlong)]),
    "pgp_get_ppf_map": (C.c_int, [C.c_void_p, _i, _i, _i, C.c_int, C.c_longlong, _i, C.POINTER(C.c_longlong)]),
    "pgp_select_bases": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, _i, _f, _i]),
    "pgp_select_bases_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, _i, _f, _i, _i]),
    "pgp_select_bases_rows_begin": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "pgp_select_bases_rows_end": (C.c_int, [C.c_void_p, _i, _f, _i, _i]),
    "pgp_ppf_features": (C.c_int, [C.c_void_p, _i, C.c_int, _i, _i]),
    "pgp_stocs_stage_weights": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, _f, _f, _i]),
    "pgp_base_invariants": (C.c_int, [C.c_void_p, _i, C.c_int, _f, _i]),
    "pgp_rigid_from_congruent": (C.c_int, [C.c_void_p, _i, _i, C.c_int, _f, _f, _f,
                                           C.POINTER(C.c_double), _i, _f]),
    "pgp_rigid_from_congruent_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _f, _f,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p]),
    "pgp_extract_pairs": (C.c_int, [C.c_void_p, C.c_float, C.c_float, _i, C.c_int, _i]),
    "pgp_find_congruent": (C.c_int, [C.c_void_p, _f, C.c_float, C.c_float, C.c_float, _i, C.c_int,
                                     _i, C.c_int, _i, C.c_int, _i]),
    "pgp_find_congruent_batch": (C.c_int, [C.c_void_p, _i, _f, _f, C.c_int, C.c_float, _i]),
    "pgp_find_congruent_batch_rows": (C.c_int, [C.c_void_p, _i, _f, _f, _i, C.c_int, C.c_float, _i]),
    "pgp_congruent_batch_quads": (C.c_int, [C.c_void_p, _i, C.c_int, _i]),
    "pgp_congruent_batch_fit": (C.c_int, [C.c_void_p, _i, _i, C.c_int, _f, _f, _f, C.POINTER(C.c_double), _i, _f]),
    "pgp_congruent_batch_fit_score": (C.c_int, [C.c_void_p, _i, _i, C.c_int, _f, _f, C.c_int, C.c_float, _f, _i, _i, _f]),
    "pgp_congruent_batch_fetch": (C.c_int, [C.c_void_p, _i, C.c_int, _f, C.POINTER(C.c_double)]),
    "pgp_congruent_batch_fit_score_list": (C.c_int, [C.c_void_p, _i, _i, C.c_int, _f, _f, C.c_int, C.c_float, C.c_int, _i, _i, _f, _f,
                                                    C.POINTER(C.c_double), _i, _i, _f, _f, C.POINTER(C.c_double), _i, _i]),
    "pgp_congruent_batch_sample_fit_score_list": (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_int, _i, _f, _f, C.c_int, C.c_float, C.c_int,
                                                           _i, _i, _f, _f, C.POINTER(C.c_double), _i, _i, _f, _f,
                                                           C.POINTER(C.c_double), _i, _i, _i, _i]),
    "pgp_sample_quads": (C.c_int, [C.c_ulonglong, _i, C.c_int, C.c_int, _i, _i]),
    "pgp_icp_refine": (C.c_int, [C.c_void_p, _f, C.c_int, _f, C.c_int, _f, C.c_int,
                                 C.POINTER(IcpParams), _f, _i]),
    "pgp_icp_refine_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_int, C.POINTER(IcpParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_icp_default_options": (C.c_int, [C.POINTER(IcpOptions)]),
    "pgp_icp_target_token": (C.c_int, [C.c_void_p, C.c_ulonglong]),
    "pgp_icp_refine_multi_device": (C.c_int, [C.POINTER(IcpJob), C.c_int, C.POINTER(IcpParams), C.c_void_p]),
    "pgp_select_top_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_set_scene_weights": (C.c_int, [C.c_void_p, _f, C.c_int]),
    "pgp_unexplained_segment": (C.c_int, [C.c_void_p, _f, C.c_int, _f, _i, _f, C.c_int, C.c_float, C.c_char_p, _i]),
    "pgp_multi_set_scene_weights": (C.c_int, [C.c_void_p, _f, C.c_int]),
    "pgp_icp_refine_ex": (C.c_int, [C.c_void_p, _f, C.c_int, _f, _f, C.c_int, _f, C.c_int,
                                    C.POINTER(IcpOptions), _f, _i]),
    "pgp_icp_refine_ex_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                           C.c_void_p, C.c_int, C.POINTER(IcpOptions), C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "pgp_radius_outlier_filter": (C.c_int, [C.c_void_p, _f, _f, C.c_int, C.c_float, C.c_int,
                                            C.POINTER(C.c_ubyte), _f, _i]),
    "pgp_backproject_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_ubyte), C.c_int, C.c_int, _f,
                                        C.c_double, C.c_double, _f, C.c_int, _i]),
    "pgp_set_scene_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]),
    "pgp_voxel_grid": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_float, _f, C.c_int, _i]),
    "pgp_mls_normals": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_float, _f, _f, _f, _i, C.c_int, _i]),
    "pgp_mls_normals_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int, _i, C.c_void_p]),
    "pgp_set_exact_records": (C.c_int, [C.c_void_p, C.c_int]),
    "pgp_set_exact_ties": (C.c_int, [C.c_void_p, C.c_int]),
    "pgp_set_verify_early_out": (C.c_int, [C.c_void_p, C.c_int]),
    "pgp_verify_early_out_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_settle_records_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "pgp_voxel_grid_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_int, _i, C.c_void_p]),
    "pgp_pose_hausdorff": (C.c_int, [C.c_void_p, _f, C.c_int, _f, C.c_int, _i, C.c_int, _f, _f]),
    "pgp_backproject_depth_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, _f,
                                               C.c_double, C.c_double, C.c_void_p, C.c_int, _i, C.c_void_p]),
    "pgp_radius_outlier_filter_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _i, C.c_void_p]),
    "pgp_center_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _f, C.c_void_p]),
    "pgp_shift_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _f, C.c_void_p]),
    "pgp_weights_from_image_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, _f, _f, C.c_void_p, C.c_int, C.c_int,
                                                C.c_void_p, C.c_void_p]),
    "pgp_segment_default_options": (C.c_int, [C.POINTER(SegmentOptions)]),
    "pgp_segment_from_depth_device": (C.c_int, [C.c_void_p, C.POINTER(SegmentOptions), C.c_void_p, C.c_int, C.c_void_p,
                                                C.c_int, C.c_int, _f, C.c_void_p, _i, _i, _f, C.c_void_p]),
    "pgp_cluster_poses_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, _f,
                                           C.POINTER(ClusterParams), C.c_void_p, C.c_void_p, _i, C.c_void_p]),
    "pgp_depth_cost": (C.c_int, [C.c_void_p, _f, _f, C.c_int, C.c_int, C.c_int, C.c_float, _f, _i]),
    "pgp_depth_cost_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_render_depth_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_int, C.POINTER(Camera), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "pgp_render_depth": (C.c_int, [C.c_void_p, _f, C.c_int, _i, C.c_int, _f, C.c_int, C.POINTER(Camera), _f, _f]),
    "pgp_cluster_poses": (C.c_int, [C.c_void_p, _f, _f, C.c_int, C.c_float, _f, C.POINTER(ClusterParams), _i,
                                    C.c_int, _i, _i]),
    "pgp_pose_error": (C.c_int, [C.c_void_p, _f, _f, C.c_int, _f, _f, _f]),
    "pgp_multi_create": (C.c_int, [C.POINTER(C.c_void_p), _i, C.c_int]),
    "pgp_multi_destroy": (C.c_int, [C.c_void_p]),
    "pgp_multi_size": (C.c_int, [C.c_void_p]),
    "pgp_multi_context": (C.c_void_p, [C.c_void_p, C.c_int]),
    "pgp_multi_slice": (C.c_int, [C.c_int, C.c_int, C.c_int, _i, _i]),
    "pgp_multi_set_scene": (C.c_int, [C.c_void_p, _f, _f, _f, C.c_int, C.c_float]),
    "pgp_multi_set_model": (C.c_int, [C.c_void_p, _f, _f, C.c_int]),
    "pgp_multi_score_lcp": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_int, C.c_float, _f, _i, _i, _f]),
    "pgp_multi_upload": (C.c_int, [C.c_void_p, _f, C.c_int]),
    "pgp_multi_score_uploaded": (C.c_int, [C.c_void_p, C.c_int, C.c_float, _f, _i, _i, _f]),
    "pgp_multi_last_timing": (C.c_int, [C.c_void_p, _f, _f, _f]),
    "pgp_multi_unique_id": (C.c_int, [C.c_void_p]),
    "pgp_multi_create_ranked": (C.c_int, [C.POINTER(C.c_void_p), _i, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pgp_multi_get_info": (C.c_int, [C.c_void_p, C.POINTER(MultiInfo)]),
    "pgp_multi_upload_slot": (C.c_int, [C.c_void_p, C.c_int, _f, C.c_int]),
    "pgp_multi_enqueue_slot": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float]),
    "pgp_multi_collect": (C.c_int, [C.c_void_p, _f, _i, _i, _f]),
    "pgp_multi_add_object": (C.c_int, [C.c_void_p]),
    "pgp_multi_objects": (C.c_int, [C.c_void_p]),
    "pgp_multi_object_context": (C.c_void_p, [C.c_void_p, C.c_int, C.c_int]),
    "pgp_multi_set_object_scene": (C.c_int, [C.c_void_p, C.c_int, _f, _f, _f, C.c_int, C.c_float]),
    "pgp_multi_set_object_scene_weights": (C.c_int, [C.c_void_p, C.c_int, _f, C.c_int]),
    "pgp_multi_set_object_model": (C.c_int, [C.c_void_p, C.c_int, _f, _f, C.c_int]),
    "pgp_multi_set_object_search_model": (C.c_int, [C.c_void_p, C.c_int, _f, C.c_int]),
    "pgp_multi_set_object_ppf_map": (C.c_int, [C.c_void_p, C.c_int, _i, _i, _i, C.c_int]),
    "pgp_multi_set_object_ppf_map_from_model": (C.c_int, [C.c_void_p, C.c_int, _f, _f, C.c_int, _i, C.POINTER(C.c_longlong)]),
    "pgp_multi_flat_slices": (C.c_int, [_i, C.c_int, C.c_int, C.c_int, _i, _i, _i, _i]),
    "pgp_multi_score_objects": (C.c_int, [C.c_void_p, C.POINTER(_f), _i, C.c_int, C.c_int, C.c_float, _f, _i, _i, _f]),
    "pgp_multi_upload_objects": (C.c_int, [C.c_void_p, C.POINTER(_f), _i, C.c_int]),
    "pgp_multi_score_objects_uploaded": (C.c_int, [C.c_void_p, C.c_int, C.c_float, _f, _i, _i, _f]),
    "pgp_multi_icp_refine": (C.c_int, [C.c_void_p, C.POINTER(MultiIcpJob), C.c_int, C.POINTER(IcpParams)]),
    "pgp_multi_find_congruent_batch": (C.c_int, [C.c_void_p, C.c_int, _i, _f, _f, C.c_int, C.c_float, _i]),
    "pgp_multi_congruent_batch_quads": (C.c_int, [C.c_void_p, C.c_int, _i, C.c_int, _i]),
    "pgp_multi_congruent_batch_fit": (C.c_int, [C.c_void_p, C.c_int, _i, _i, C.c_int, _f, _f, _f, C.POINTER(C.c_double), _i, _f]),
    "pgp_set_kernel_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "pgp_get_kernel_timing": (C.c_int, [C.c_void_p, _i, _f, C.c_int]),
    "pgp_get_index_info": (C.c_int, [C.c_void_p, C.POINTER(IndexInfo)]),
    "pgp_set_nn_pruning": (C.c_int, [C.c_void_p, C.c_int]),
    "pgp_get_nn_lists_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong),
                                        C.POINTER(C.c_longlong), C.POINTER(C.c_float)]),
    "pgp_plane_default_options": (C.c_int, [C.POINTER(PlaneOptions)]),
    "pgp_fit_plane": (C.c_int, [C.c_void_p, _f, C.c_int, C.POINTER(PlaneOptions), _i, C.c_int, _f, C.POINTER(C.c_ubyte), _i,
                                C.POINTER(PlaneInfo)]),
    "pgp_fit_plane_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(PlaneOptions), C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_mask_plane_depth": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _f, _f, C.c_double, _i]),
    "pgp_mask_plane_depth_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _f, _f, C.c_double,
                                              C.c_void_p, C.c_void_p]),
    "pgp_remove_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _f, C.c_float,
                                   C.POINTER(PlaneOptions), _f, _i]),
    "pgp_components_default_options": (C.c_int, [C.POINTER(ComponentsOptions)]),
    "pgp_depth_components": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                       C.c_int, _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _i]),
    "pgp_depth_components_device": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_int, C.c_int, _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p]),
    "pgp_component_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "pgp_component_mask_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "pgp_assign_masks_to_components": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _i, C.c_int,
                                                 _i, _i, _i, _i]),
    "pgp_assign_masks_to_components_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, _i,
                                                        C.c_int, _i, _i, _i, _i, C.c_void_p]),
    "pgp_crease_default_options": (C.c_int, [C.POINTER(CreaseOptions)]),
    # ctx, options, crease options, image, raw16, mask, rows, cols, K, outputs ...
    "pgp_depth_normals": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.POINTER(CreaseOptions), C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_int, _f, C.c_void_p]),
    "pgp_depth_normals_device": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.POINTER(CreaseOptions), C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_int, _f, C.c_void_p, C.c_void_p]),
    "pgp_depth_crease_mask": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.POINTER(CreaseOptions), C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_int, C.c_int, _f, C.c_void_p, _i]),
    "pgp_depth_crease_mask_device": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.POINTER(CreaseOptions), C.c_void_p,
                                               C.c_int, C.c_void_p, C.c_int, C.c_int, _f, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_depth_objects": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.POINTER(CreaseOptions), C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_int, _f, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _i]),
    "pgp_depth_objects_device": (C.c_int, [C.c_void_p, C.POINTER(ComponentsOptions), C.POINTER(CreaseOptions), C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_int, C.c_int, _f, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int, C.c_void_p, C.c_void_p]),
    "pgp_ppf_default_options": (C.c_int, [C.POINTER(PpfOptions)]),
    "pgp_set_ppf_model": (C.c_int, [C.c_void_p, _f, _f, C.c_int]),
    "pgp_ppf_vote_device": (C.c_int, [C.c_void_p, C.POINTER(PpfOptions), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p, C.c_void_p]),
    "pgp_ppf_vote": (C.c_int, [C.c_void_p, C.POINTER(PpfOptions), _f, _i, _i, _i, C.c_int, _i]),
    "pgp_ppf_hypotheses": (C.c_int, [C.c_void_p, C.POINTER(PpfOptions), C.c_int, C.c_float, _f, _f, _i, C.c_int, _i, _i, _f,
                                     _f]),
    "pgp_ppf_accumulator": (C.c_int, [C.c_void_p, C.POINTER(PpfOptions), _i, C.c_int, _i]),
    "pgp_ppf_model_angles": (C.c_int, [C.c_void_p, _f, C.c_longlong]),
    "pgp_select_tetrahedron_bases": (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_int, C.c_int, C.c_int, C.c_float, _i, _f, _i]),
    "pgp_find_congruent_v4pcs": (C.c_int, [C.c_void_p, _f, C.c_float, _i, C.c_int, C.POINTER(C.c_longlong)]),
    "pgp_find_congruent_v4pcs_batch": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_longlong), _i]),
    "pgp_v4pcs_batch_quads": (C.c_int, [C.c_void_p, _i, C.c_int, _i]),
    "pgp_v4pcs_default_options": (C.c_int, [C.POINTER(V4pcsOptions)]),
    "pgp_v4pcs_hypotheses": (C.c_int, [C.c_void_p, C.POINTER(V4pcsOptions), _f, _f, _i, _i, _i, _f, C.POINTER(C.c_double), _i, _f,
                                       _i, _i, _f, _f, C.POINTER(C.c_double)]),
    "pgp_select_wide_bases": (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_int, C.c_int, C.c_float, _i, _f, _f, _i]),
    "pgp_extract_pairs_batch": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_float, _i]),
    "pgp_extract_pairs_batch_fetch": (C.c_int, [C.c_void_p, C.c_int, _i, C.c_int, _i]),
    "pgp_find_congruent_batch_lists": (C.c_int, [C.c_void_p, _f, _f, _i, C.c_int, C.c_float, _i]),
    "pgp_super4pcs_default_options": (C.c_int, [C.POINTER(Super4pcsOptions)]),
    "pgp_super4pcs_hypotheses": (C.c_int, [C.c_void_p, C.POINTER(Super4pcsOptions), _f, _f, _i, _i, _f, _i, _f, C.POINTER(C.c_double),
                                           _i, _f, _i, _i, _f, _f, C.POINTER(C.c_double)]),
    "pgp_set_scene_colors": (C.c_int, [C.c_void_p, _f, C.c_int]),
    "pgp_set_search_model_attributes": (C.c_int, [C.c_void_p, _f, _f, C.c_int]),
    "pgp_pair_gates_default": (C.c_int, [C.POINTER(PairGates)]),
    "pgp_extract_pairs_batch_gated": (C.c_int, [C.c_void_p, _f, _i, C.c_int, C.c_float, C.POINTER(PairGates), _i]),
    "pgp_super4pcs_hypotheses_gated": (C.c_int, [C.c_void_p, C.POINTER(Super4pcsOptions), C.POINTER(PairGates), _f, _f, _i, _i, _f, _i,
                                                 _f, C.POINTER(C.c_double), _i, _f, _i, _i, _f, _f, C.POINTER(C.c_double)]),
    "pgp_physics_default_options": (C.c_int, [C.POINTER(PhysicsOptions)]),
    "pgp_convex_hull": (C.c_int, [_f, C.c_int, C.c_int, _f, _i, _f, _i]),
    "pgp_physics_add_shape": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_float, C.c_int, _i]),
    "pgp_physics_shape_info": (C.c_int, [C.c_void_p, C.c_int, _f, _i, _f, _i, _f, _f]),
    "pgp_physics_shape_edges": (C.c_int, [C.c_void_p, C.c_int, _i, _i]),
    "pgp_physics_set_edge_contacts": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "pgp_physics_shape_faces": (C.c_int, [C.c_void_p, C.c_int, _i, _i, _i]),
    "pgp_physics_set_polyhedral_contacts": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "pgp_physics_settle": (C.c_int, [C.c_void_p, C.POINTER(PhysicsOptions), C.c_int, _i, _f, _i, _i, _f, _f, _f, _f,
                                     C.POINTER(PhysicsInfo)]),
    "pgp_physics_settle_device": (C.c_int, [C.c_void_p, C.POINTER(PhysicsOptions), C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, _f, _f, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "pgp_physics_trace": (C.c_int, [C.c_void_p, C.POINTER(PhysicsOptions), C.c_int, _f, C.c_int, _i, _f, _f, _f, _f, _f,
                                    _i]),
    "pgp_mcts_default_options": (C.c_int, [C.c_void_p]),
    "pgp_mcts_search": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _f, _f, C.POINTER(Camera), _f, _i, _f, _f,
                                  C.c_void_p, C.c_void_p, C.c_int, _i]),
    "pgp_tricp_default_options": (C.c_int, [C.POINTER(TricpOptions)]),
    "pgp_tricp_set_objects": (C.c_int, [C.c_void_p, C.POINTER(TricpObject), C.c_int]),
    "pgp_tricp_states": (C.c_int, [C.c_void_p, C.POINTER(TricpOptions), C.c_int, _i, _f, _i, _i, _f, _f, _i, _i]),
    "pgp_tricp_states_device": (C.c_int, [C.c_void_p, C.POINTER(TricpOptions), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_mcts_set_tricp": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(TricpOptions)]),
    "pgp_sample_mesh": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_int, _i, C.c_int, C.c_int, C.c_ulonglong, _f, _f, _i]),
    "pgp_sample_mesh_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_ulonglong,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "pgp_farthest_points": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_int, C.c_int, _i, _f]),
    "pgp_farthest_points_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "pgp_model_from_mesh": (C.c_int, [C.c_void_p, _f, C.c_int, C.c_int, _i, C.c_int, C.c_int, C.c_int, C.c_ulonglong, _f, _f, _i,
                                      _f]),
}

_lib = None


def load():
    """Load libpgp.so and bind every declared symbol; raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `make -C physimglobalpose_amd/csrc` "
            "(or __graft_entry__.build()); there is no fallback path")
    # PyTorch-ROCm wheels bundle their own libamdhip64; if libpgp.so pulls in the system HIP
    # runtime first, a later `import torch` finds two runtimes in the process and reports
    # "No HIP GPUs are available".  Loading torch first makes both share one runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class PgpError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        msg = load().pgp_last_error()
        raise PgpError(f"libpgp error {rc}: {msg.decode() if msg else '?'}")
