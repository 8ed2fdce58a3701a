"""ctypes binding of include/rgbd360_hip.h.  Loading fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RGBD360_LIB") or os.path.join(_HERE, "lib", "librgbd360_hip.so")     # RGBD360_LIB: another build of the library (A/B runs)

# Every symbol include/rgbd360_hip.h declares (checked by tests/test_abi.py against the header text).
SYMBOLS = [
    "rgbd360_default_params", "rgbd360_create", "rgbd360_destroy", "rgbd360_last_error", "rgbd360_set_target",
    "rgbd360_set_source", "rgbd360_set_target_dev", "rgbd360_set_source_dev", "rgbd360_promote_source_to_target",
    "rgbd360_align360", "rgbd360_align360_begin", "rgbd360_align360_finish", "rgbd360_align360_batch", "rgbd360_align360_batch_dev", "rgbd360_level_dims", "rgbd360_get_plane", "rgbd360_get_lut", "rgbd360_eval", "rgbd360_eval_occ",
    "rgbd360_warp_indices", "rgbd360_gn_step", "rgbd360_forced_iters", "rgbd360_time_eval_kernel", "rgbd360_stream",
    "rgbd360_sync", "rgbd360_device_count", "rgbd360_sphere_cloud", "rgbd360_selftest_math", "rgbd360_selftest_libm", "rgbd360_set_index_arithmetic", "rgbd360_get_index_arithmetic", "rgbd360_time_solve_kernel", "rgbd360_normals", "rgbd360_distance_map",
    "rgbd360_plane_fit", "rgbd360_frame_planes", "rgbd360_frame_planes_dev", "rgbd360_load_frame_bin", "rgbd360_stitch_sphere",
    "rgbd360_set_camera", "rgbd360_align_pinhole", "rgbd360_eval_pinhole", "rgbd360_eval_pinhole_occ", "rgbd360_use_saliency", "rgbd360_warp_indices_pinhole",
    "rgbd360_pbmap_default_params", "rgbd360_register_planes", "rgbd360_bilateral_filter",
    "rgbd360_cloud_planes", "rgbd360_sensor_cloud", "rgbd360_sensor_planes", "rgbd360_sensor_planes_ex", "rgbd360_sensor_cloud_ex", "rgbd360_depth_model_load", "rgbd360_depth_model_free", "rgbd360_depth_model_info", "rgbd360_depth_model_undistort", "rgbd360_merge_planes", "rgbd360_group_planes", "rgbd360_pool_sensor_planes", "rgbd360_debug_set_schedule", "rgbd360_debug_set_sequence_route", "rgbd360_debug_knobs_enabled", "rgbd360_frame_planes_stage_timing", "rgbd360_frame_planes_stage_times", "rgbd360_planes_available", "rgbd360_set_plane_refinement", "rgbd360_plane_refinement_stats", "rgbd360_debug_plane_sums", "rgbd360_set_plane_color_image",
    "rgbd360_multi_create", "rgbd360_multi_destroy", "rgbd360_multi_last_error", "rgbd360_multi_n_gpus", "rgbd360_multi_uses_rccl", "rgbd360_multi_set_index_arithmetic",
    "rgbd360_shard_range", "rgbd360_gather_slot", "rgbd360_multi_align_sequence", "rgbd360_multi_load_sequence", "rgbd360_multi_align_resident",
    "rgbd360_align360_batch_multi", "rgbd360_time_eval_kernel_rotating", "rgbd360_forced_iters_batch",
    "rgbd360_rig_create", "rgbd360_rig_destroy", "rgbd360_rig_last_error", "rgbd360_rig_set_target", "rgbd360_rig_set_source",
    "rgbd360_rig_eval", "rgbd360_rig_align", "rgbd360_rig_use_saliency", "rgbd360_rig_set_index_arithmetic", "rgbd360_rig_get_index_arithmetic",
    "rgbd360_rig_warp_indices", "rgbd360_debug_solve_partials",
    "rgbd360_debug_solve_state", "rgbd360_debug_solve_table",
    "rgbd360_store_create", "rgbd360_store_destroy", "rgbd360_store_last_error", "rgbd360_store_entry_bytes", "rgbd360_store_put",
    "rgbd360_store_occupied", "rgbd360_store_align",
    "rgbd360_store_overlap_default_params", "rgbd360_store_overlap", "rgbd360_store_overlap_all", "rgbd360_overlap_candidates",
    "rgbd360_overlap_representative", "rgbd360_store_time_overlap", "rgbd360_store_time_overlap_all",
    "rgbd360_warp_images", "rgbd360_warp_images_dev", "rgbd360_warp_images_pinhole", "rgbd360_time_warp_images",
    "rgbd360_map_create", "rgbd360_map_destroy", "rgbd360_map_last_error", "rgbd360_map_bytes", "rgbd360_map_set_box",
    "rgbd360_map_insert_sphere", "rgbd360_map_insert_cloud", "rgbd360_map_size", "rgbd360_map_clear", "rgbd360_map_extract",
    "rgbd360_map_extract_dev", "rgbd360_map_time_kernels",
    "rgbd360_map_remove_sphere", "rgbd360_map_remove_cloud", "rgbd360_map_move_sphere", "rgbd360_map_move_cloud", "rgbd360_map_rehash",
    "rgbd360_map_census", "rgbd360_map_time_edit",
    "rgbd360_map_default_align_params", "rgbd360_map_align_sphere", "rgbd360_map_align_cloud", "rgbd360_map_align_eval", "rgbd360_map_time_align",
    "rgbd360_map_default_align_plane_params", "rgbd360_map_align_plane_sphere", "rgbd360_map_align_plane_cloud", "rgbd360_map_align_plane_eval",
    "rgbd360_map_plane_fit", "rgbd360_map_time_align_plane",
    "rgbd360_map_align_batch_cloud", "rgbd360_map_align_batch_sphere", "rgbd360_map_align_plane_batch_cloud", "rgbd360_map_align_plane_batch_sphere",
    "rgbd360_map_align_best", "rgbd360_map_align_plane_best", "rgbd360_map_align_batch_trace",
    "rgbd360_map_default_rig_calib_params", "rgbd360_map_calibrate_rig_clouds", "rgbd360_map_calibrate_rig_depth", "rgbd360_rig_save_extrinsics",
    "rgbd360_rig_calib_solve_host", "rgbd360_rig_calib_solve_dev", "rgbd360_rig_calib_trace", "rgbd360_rig_calib_time_solve",
    "rgbd360_map_default_align_gicp_params", "rgbd360_map_align_gicp_sphere", "rgbd360_map_align_gicp_cloud", "rgbd360_map_align_gicp_eval",
    "rgbd360_map_gicp_weight", "rgbd360_map_time_align_gicp",
    "rgbd360_map_default_colour_params", "rgbd360_map_colours", "rgbd360_map_colours_dev", "rgbd360_map_colour_bytes", "rgbd360_map_release_colours",
    "rgbd360_map_colour_gradient", "rgbd360_map_colour_intensity", "rgbd360_map_time_colours",
    "rgbd360_map_default_align_colour_params", "rgbd360_map_align_colour_sphere", "rgbd360_map_align_colour_cloud", "rgbd360_map_align_colour_eval",
    "rgbd360_map_time_align_colour",
    "rgbd360_map_set_align_robust", "rgbd360_map_get_align_robust", "rgbd360_map_align_robust_info", "rgbd360_map_align_batch_robust_info",
    "rgbd360_map_align_robust_eval", "rgbd360_map_time_align_robust",
    "rgbd360_map_default_render_params", "rgbd360_map_render_sphere", "rgbd360_map_render_sphere_dev", "rgbd360_map_time_render",
    "rgbd360_map_default_raycast_params", "rgbd360_map_raycast", "rgbd360_map_raycast_sphere", "rgbd360_map_raycast_sphere_dev",
    "rgbd360_map_raycast_set_plain", "rgbd360_map_time_raycast",
    "rgbd360_map_default_normal_params", "rgbd360_map_normals", "rgbd360_map_normals_dev", "rgbd360_map_raycast_surface",
    "rgbd360_map_raycast_surface_sphere", "rgbd360_map_raycast_surface_sphere_dev", "rgbd360_map_time_normals",
    "rgbd360_map_default_observe_params", "rgbd360_map_observe_sphere", "rgbd360_map_observe_rays", "rgbd360_map_votes", "rgbd360_map_carve",
    "rgbd360_map_vote_bytes", "rgbd360_map_release_votes", "rgbd360_map_time_observe",
    "rgbd360_map_level", "rgbd360_map_pyramid_bytes", "rgbd360_map_release_levels", "rgbd360_map_default_c2f_params",
    "rgbd360_map_align_c2f_sphere", "rgbd360_map_align_c2f_cloud", "rgbd360_map_time_coarsen",
    "rgbd360_map_default_merge_params", "rgbd360_map_merge", "rgbd360_map_unmerge", "rgbd360_map_records", "rgbd360_map_add_records",
    "rgbd360_map_time_merge",
    "rgbd360_map_default_plane_seg_params", "rgbd360_map_planes", "rgbd360_map_plane_labels", "rgbd360_map_plane_bytes",
    "rgbd360_map_release_planes", "rgbd360_map_plane_from_sums", "rgbd360_map_plane_from_members", "rgbd360_map_plane_sums_in_range",
    "rgbd360_map_time_planes",
    "rgbd360_graph_create", "rgbd360_graph_destroy", "rgbd360_graph_last_error", "rgbd360_graph_add_vertices", "rgbd360_graph_add_edges",
    "rgbd360_graph_set_poses", "rgbd360_graph_set_fixed", "rgbd360_graph_n_vertices", "rgbd360_graph_n_edges", "rgbd360_graph_clear",
    "rgbd360_graph_default_params", "rgbd360_graph_optimize", "rgbd360_graph_get_poses", "rgbd360_graph_chi2", "rgbd360_graph_get_trace",
    "rgbd360_graph_linearize", "rgbd360_graph_apply", "rgbd360_graph_time_kernels",
    "rgbd360_graph_set_edge_robust", "rgbd360_graph_set_edge_enabled", "rgbd360_graph_get_edge_state", "rgbd360_graph_edge_weights",
    "rgbd360_graph_default_cov_params", "rgbd360_graph_marginals", "rgbd360_graph_relative_covariances", "rgbd360_graph_time_cov_kernels",
    "rgbd360_depth_trainer_create", "rgbd360_depth_trainer_destroy", "rgbd360_depth_trainer_last_error", "rgbd360_depth_trainer_clear",
    "rgbd360_depth_default_train_params", "rgbd360_depth_trainer_accumulate_images", "rgbd360_depth_trainer_accumulate_map",
    "rgbd360_depth_trainer_sums", "rgbd360_depth_trainer_add_sums", "rgbd360_depth_trainer_model", "rgbd360_depth_model_from_sums",
    "rgbd360_depth_model_save", "rgbd360_depth_trainer_set_form", "rgbd360_depth_trainer_time_map",
    "rgbd360_depth_models_create", "rgbd360_depth_models_destroy", "rgbd360_depth_models_bytes", "rgbd360_depth_models_set",
    "rgbd360_depth_undistort", "rgbd360_rig_depth_clouds", "rgbd360_map_calibrate_rig_depth_models", "rgbd360_depth_evaluate_map",
    "rgbd360_depth_models_pack", "rgbd360_depth_models_repack", "rgbd360_depth_models_undistort_packed_host",
    "rgbd360_depth_apply_timing", "rgbd360_depth_apply_last_us", "rgbd360_depth_apply_time_copy",
]


class Params(C.Structure):
    _fields_ = [("n_pyr", C.c_int), ("min_depth", C.c_float), ("max_depth", C.c_float), ("sigma_photo", C.c_float),
                ("sigma_depth", C.c_float), ("thres_sal_photo", C.c_float), ("thres_sal_depth", C.c_float),
                ("max_iters", C.c_int), ("tol_residual", C.c_float), ("tol_update", C.c_float), ("mask_seams", C.c_int),
                ("device", C.c_int)]


class Result(C.Structure):
    _fields_ = [("status", C.c_int), ("iters", C.c_int * 8), ("sso", C.c_float), ("err_final", C.c_double),
                ("rms_photo", C.c_double), ("rms_depth", C.c_double), ("hessian", C.c_float * 36),
                ("gradient", C.c_float * 6)]


class SolveStateIn(C.Structure):       # rgbd360_solve_state_in (rgbd360_hip_diag.h)
    _fields_ = [("pose", C.c_float * 16), ("update", C.c_float * 6), ("lambda_", C.c_double), ("error", C.c_double),
                ("first", C.c_int), ("it", C.c_int), ("max_iters", C.c_int), ("forced", C.c_int),
                ("tol_residual", C.c_double), ("tol_update", C.c_double)]


class SolveStateOut(C.Structure):      # rgbd360_solve_state_out
    _fields_ = [("status", C.c_int), ("done", C.c_int), ("level_active", C.c_int), ("it", C.c_int), ("n_evals", C.c_int),
                ("pend_nb", C.c_int), ("iters_level", C.c_int), ("cand", C.c_float * 16), ("pose", C.c_float * 16),
                ("update", C.c_float * 6), ("lambda_", C.c_double), ("error", C.c_double), ("new_error", C.c_double),
                ("diff_error", C.c_double)]


class Plane(C.Structure):
    _fields_ = [("centroid", C.c_float * 3), ("normal", C.c_float * 3), ("d", C.c_float), ("curvature", C.c_float),
                ("count", C.c_int), ("root", C.c_int), ("area", C.c_float), ("elongation", C.c_float),
                ("ppal_dir", C.c_float * 3), ("area_moment", C.c_float), ("center_hull", C.c_float * 3), ("hull_points", C.c_int),
                ("color_count", C.c_int), ("color_nrgb", C.c_float * 3), ("color_dev", C.c_float * 3), ("intensity", C.c_float),
                ("hist_h", C.c_float * 74), ("hull_n", C.c_int), ("hull", (C.c_float * 3) * 64),
                ("color_mode_count", C.c_int), ("color_mode", C.c_float * 3), ("intensity_mode", C.c_float), ("color_concentration", C.c_float)]


class MapStats(C.Structure):       # rgbd360_map_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_valid", "n_box_rejected", "n_out_of_range", "n_added", "n_dropped_full", "n_voxels")]


class MapEditStats(C.Structure):   # rgbd360_map_edit_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_valid", "n_box_rejected", "n_out_of_range", "n_removed", "n_missing", "n_underflow",
                                            "n_voxels_emptied", "n_voxels")]


class MapCensus(C.Structure):      # rgbd360_map_census_counts
    _fields_ = [(n, C.c_longlong) for n in ("n_slots", "n_live", "n_tombstones", "n_points", "n_inconsistent")]


class MapAlignParams(C.Structure):       # rgbd360_map_align_params
    _fields_ = [("max_dist", C.c_float), ("max_iters", C.c_int), ("eps", C.c_float), ("min_count", C.c_int), ("min_matches", C.c_longlong)]


class MapAlignResult(C.Structure):       # rgbd360_map_align_result
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("converged", C.c_int), ("n_valid", C.c_longlong), ("n_box_rejected", C.c_longlong),
                ("n_out_of_range", C.c_longlong), ("n_matched", C.c_longlong), ("fitness", C.c_double), ("hessian", C.c_float * 36),
                ("gradient", C.c_float * 6)]


class MapAlignPlaneParams(C.Structure):  # rgbd360_map_align_plane_params
    _fields_ = MapAlignParams._fields_ + [("min_support", C.c_int), ("max_flatness", C.c_float)]


class MapAlignPlaneResult(C.Structure):  # rgbd360_map_align_plane_result
    _fields_ = MapAlignResult._fields_ + [("n_unsupported", C.c_longlong), ("n_nonplanar", C.c_longlong), ("fitness_point", C.c_double)]


class MapAlignGicpParams(C.Structure):   # rgbd360_map_align_gicp_params
    _fields_ = MapAlignParams._fields_ + [("epsilon", C.c_float), ("use_target_normals", C.c_int), ("min_support", C.c_int), ("max_flatness", C.c_float)]


class MapAlignGicpResult(C.Structure):   # rgbd360_map_align_gicp_result
    _fields_ = MapAlignResult._fields_ + [("n_target_planes", C.c_longlong), ("n_source_planes", C.c_longlong), ("n_plane_pairs", C.c_longlong),
                                          ("fitness_point", C.c_double)]


class MapColourParams(C.Structure):      # rgbd360_map_colour_params
    _fields_ = [("min_count", C.c_int), ("min_support", C.c_int), ("max_flatness", C.c_float), ("min_gradient_support", C.c_int), ("min_spread", C.c_float)]


class MapColourStats(C.Structure):       # rgbd360_map_colour_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_voxels", "n_below_min_count", "n_no_normal", "n_no_gradient", "n_gradients")]


class MapAlignColourParams(C.Structure):     # rgbd360_map_align_colour_params
    _fields_ = MapAlignParams._fields_ + [("lambda_geometric", C.c_float), ("min_support", C.c_int), ("max_flatness", C.c_float),
                                          ("min_gradient_support", C.c_int), ("min_spread", C.c_float)]


class MapAlignColourResult(C.Structure):     # rgbd360_map_align_colour_result
    _fields_ = MapAlignResult._fields_ + [("n_no_normal", C.c_longlong), ("n_no_gradient", C.c_longlong), ("rms_geometric", C.c_double),
                                          ("rms_colour", C.c_double)]


class MapRobust(C.Structure):            # rgbd360_map_robust
    _fields_ = [("kind", C.c_int), ("scale_with_level", C.c_int), ("delta", C.c_double)]


class MapRobustInfo(C.Structure):        # rgbd360_map_robust_info
    _fields_ = [("method", C.c_int), ("kind", C.c_int), ("delta_eff", C.c_double), ("sum_w", C.c_double), ("n", C.c_longlong), ("n_downweighted", C.c_longlong)]


MAP_METHOD_POINT, MAP_METHOD_PLANE, MAP_METHOD_GICP, MAP_METHOD_COLOUR = 0, 1, 2, 3                     # RGBD360_MAP_METHOD_*
MAP_ROBUST_NONE, MAP_ROBUST_HUBER, MAP_ROBUST_CAUCHY, MAP_ROBUST_GEMAN_MCCLURE = 0, 1, 2, 3             # RGBD360_MAP_ROBUST_*


class MapAlignTrace(C.Structure):        # rgbd360_map_align_trace (rgbd360_hip_diag.h)
    _fields_ = [("n", C.c_longlong), ("sum_sq", C.c_double), ("update", C.c_float * 6)]


MAP_BATCH_MAX = 1024                     # RGBD360_MAP_BATCH_MAX


class MapBatchCloud(C.Structure):        # rgbd360_map_batch_cloud
    _fields_ = [("xyz", C.c_void_p), ("n", C.c_longlong)]


class MapBatchFrame(C.Structure):        # rgbd360_map_batch_frame
    _fields_ = [("depth", C.c_void_p), ("depth_step", C.c_size_t)]


class MapBatchJob(C.Structure):          # rgbd360_map_batch_job
    _fields_ = [("input", C.c_int), ("guess", C.c_float * 16)]


RIG_CALIB_MAX_SENSORS = 16               # RGBD360_RIG_CALIB_MAX_SENSORS


class RigCalibParams(C.Structure):       # rgbd360_rig_calib_params
    _fields_ = [("plane", MapAlignPlaneParams), ("refine_poses", C.c_int), ("fixed_sensor", C.c_int), ("lambda_", C.c_float),
                ("min_input_matches", C.c_longlong)]


class RigCalibResult(C.Structure):       # rgbd360_rig_calib_result
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("converged", C.c_int), ("n_inputs_used", C.c_int), ("n_frames_skipped", C.c_int),
                ("n_matched", C.c_longlong), ("cost", C.c_double), ("fitness", C.c_double)]


class RigCalibSensor(C.Structure):       # rgbd360_rig_calib_sensor
    _fields_ = [("n_matched", C.c_longlong), ("cost", C.c_double), ("hessian", C.c_float * 36), ("gradient", C.c_float * 6)]


class RigCalibStep(C.Structure):         # rgbd360_rig_calib_step (rgbd360_hip_diag.h)
    _fields_ = [("n", C.c_longlong), ("cost", C.c_double), ("max_vv", C.c_float), ("max_ww", C.c_float)]


MAP_MAX_SHIFT = 6                        # RGBD360_MAP_MAX_SHIFT


class MapC2fParams(C.Structure):         # rgbd360_map_c2f_params
    _fields_ = [("top_shift", C.c_int), ("kind", C.c_int), ("max_iters", C.c_int), ("min_count", C.c_int), ("eps", C.c_float),
                ("max_dist_leaves", C.c_float), ("min_matches", C.c_longlong), ("min_support", C.c_int), ("max_flatness", C.c_float)]


class MapC2fLevel(C.Structure):          # rgbd360_map_c2f_level
    _fields_ = [("shift", C.c_int), ("status", C.c_int), ("iterations", C.c_int), ("converged", C.c_int), ("n_valid", C.c_longlong),
                ("n_box_rejected", C.c_longlong), ("n_out_of_range", C.c_longlong), ("n_matched", C.c_longlong), ("fitness", C.c_double),
                ("pose", C.c_float * 16)]


class MapC2fResult(C.Structure):         # rgbd360_map_c2f_result
    _fields_ = [("n_levels", C.c_int), ("levels", MapC2fLevel * (MAP_MAX_SHIFT + 1)), ("hessian", C.c_float * 36), ("gradient", C.c_float * 6)]


class MapMergeParams(C.Structure):      # rgbd360_map_merge_params
    _fields_ = [("min_count", C.c_int)]


class MapMergeStats(C.Structure):       # rgbd360_map_merge_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_voxels_read", "n_points_read", "n_voxels_below_min_count", "n_points_below_min_count",
                                            "n_voxels_out_of_range", "n_points_out_of_range", "n_voxels_added", "n_points_added", "n_voxels_new",
                                            "n_voxels_dropped", "n_points_dropped", "n_missing", "n_underflow", "n_voxels")]


class MapRenderParams(C.Structure):     # rgbd360_map_render_params
    _fields_ = [("min_count", C.c_int), ("near", C.c_float), ("splat", C.c_float), ("max_half", C.c_int)]


class MapRenderStats(C.Structure):      # rgbd360_map_render_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_voxels", "n_below_min_count", "n_near", "n_splatted", "n_pixels_covered")]


class MapRaycastParams(C.Structure):    # rgbd360_map_raycast_params
    _fields_ = [("min_count", C.c_int), ("t_min", C.c_float), ("t_max", C.c_float), ("max_offset", C.c_float), ("max_steps", C.c_int)]


class MapRaycastStats(C.Structure):     # rgbd360_map_raycast_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_rays", "n_hits", "n_miss_box", "n_left_box", "n_t_max", "n_max_steps", "n_bad_rays", "n_steps",
                                            "n_lookups")]


class MapNormalParams(C.Structure):     # rgbd360_map_normal_params
    _fields_ = [("min_count", C.c_int), ("min_support", C.c_int), ("max_flatness", C.c_float), ("max_shift", C.c_float)]


class DepthTrainParams(C.Structure):    # rgbd360_depth_train_params
    _fields_ = [("ray", MapRaycastParams), ("normal", MapNormalParams), ("require_plane", C.c_int), ("min_cos_incidence", C.c_float),
                ("min_mult", C.c_float), ("max_mult", C.c_float), ("max_range", C.c_float)]


class DepthTrainStats(C.Structure):     # rgbd360_depth_train_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_pixels", "n_no_measurement", "n_no_hit", "n_off_plane", "n_grazing", "n_out_of_range",
                                            "n_mult_rejected", "n_examples")]


class DepthEvalSums(C.Structure):       # rgbd360_depth_eval_sums
    _fields_ = [(n, C.c_longlong) for n in ("n", "raw_e", "raw_ee", "cor_e", "cor_ee")]


class MapNormalStats(C.Structure):      # rgbd360_map_normal_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_voxels", "n_below_min_count", "n_unsupported", "n_nonplanar", "n_normals")]


class MapPlaneSegParams(C.Structure):   # rgbd360_map_plane_seg_params
    _fields_ = [("min_count", C.c_int), ("min_support", C.c_int), ("max_flatness", C.c_float), ("max_voxel_curvature", C.c_float),
                ("cos_angle", C.c_float), ("max_offset", C.c_float), ("min_voxels", C.c_int), ("max_curvature", C.c_float)]


class MapPlaneSegStats(C.Structure):    # rgbd360_map_plane_seg_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_voxels", "n_eligible", "n_links", "n_regions", "n_planes_available", "n_voxels_in_planes")]


# RGBD360_MAP_PLANE_DIRS: the 64 in-plane directions of a map plane's hull, (a_k, b_k) about 1024 (cos, sin) of 2 pi k / 64
MAP_PLANE_DIRS = (
    (1024, 0), (1019, 100), (1004, 200), (980, 297), (946, 392), (903, 483), (851, 569), (792, 650), (724, 724), (650, 792), (569, 851),
    (483, 903), (392, 946), (297, 980), (200, 1004), (100, 1019), (0, 1024), (-100, 1019), (-200, 1004), (-297, 980), (-392, 946),
    (-483, 903), (-569, 851), (-650, 792), (-724, 724), (-792, 650), (-851, 569), (-903, 483), (-946, 392), (-980, 297), (-1004, 200),
    (-1019, 100), (-1024, 0), (-1019, -100), (-1004, -200), (-980, -297), (-946, -392), (-903, -483), (-851, -569), (-792, -650),
    (-724, -724), (-650, -792), (-569, -851), (-483, -903), (-392, -946), (-297, -980), (-200, -1004), (-100, -1019), (0, -1024),
    (100, -1019), (200, -1004), (297, -980), (392, -946), (483, -903), (569, -851), (650, -792), (724, -724), (792, -650), (851, -569),
    (903, -483), (946, -392), (980, -297), (1004, -200), (1019, -100))


class MapObserveParams(C.Structure):    # rgbd360_map_observe_params
    _fields_ = [("min_count", C.c_int), ("near", C.c_float), ("margin_leaves", C.c_float), ("margin_rel", C.c_float), ("max_offset", C.c_float),
                ("max_steps", C.c_int), ("accumulate", C.c_int)]


class MapObserveStats(C.Structure):     # rgbd360_map_observe_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_rays", "n_valid", "n_skipped", "n_miss_box", "n_max_steps", "n_steps", "n_lookups", "n_through", "n_end",
                                            "n_voxels_voted")]


class MapCarveStats(C.Structure):       # rgbd360_map_carve_stats
    _fields_ = [(n, C.c_longlong) for n in ("n_voted", "n_voxels_carved", "n_points_carved", "n_protected_end", "n_protected_count", "n_voxels")]


class GraphParams(C.Structure):         # rgbd360_graph_params
    _fields_ = [("max_iters", C.c_int), ("cg_max_iters", C.c_int), ("tol_update", C.c_double), ("lambda_init", C.c_double),
                ("lambda_max", C.c_double), ("cg_tol", C.c_double)]


class GraphResult(C.Structure):         # rgbd360_graph_result
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("accepted", C.c_int), ("converged", C.c_int), ("chi2_initial", C.c_double),
                ("chi2_final", C.c_double), ("lambda_final", C.c_double), ("cg_iterations", C.c_longlong), ("n_fixed", C.c_int),
                ("n_isolated", C.c_int)]


class GraphIteration(C.Structure):      # rgbd360_graph_iteration
    _fields_ = [("chi2", C.c_double), ("chi2_trial", C.c_double), ("lambda_", C.c_double), ("accepted", C.c_int), ("cg_iterations", C.c_int),
                ("cg_residual", C.c_double), ("max_update", C.c_double)]


class GraphCovParams(C.Structure):      # rgbd360_graph_cov_params
    _fields_ = [("cg_max_iters", C.c_int), ("cg_tol", C.c_double)]


class GraphCovResult(C.Structure):      # rgbd360_graph_cov_result
    _fields_ = [("status", C.c_int), ("n_queries", C.c_int), ("n_not_converged", C.c_int), ("cg_iterations_max", C.c_int),
                ("cg_residual_max", C.c_double), ("dof", C.c_longlong), ("cost", C.c_double), ("variance_factor", C.c_double),
                ("n_fixed", C.c_int), ("n_isolated", C.c_int)]


class OverlapParams(C.Structure):        # rgbd360_overlap_params
    _fields_ = [("level", C.c_int), ("tol_abs", C.c_float), ("tol_rel", C.c_float)]


# rgbd360_overlap as a numpy record (eight int32)
OVERLAP_FIELDS = ("evaluated", "n_valid", "n_visible", "n_target", "n_consistent", "n_behind", "n_in_front", "reserved")


class PbmapParams(C.Structure):
    _fields_ = [("dist_d", C.c_float), ("angle_deg", C.c_float), ("elongation_threshold", C.c_float),
                ("area_threshold", C.c_float), ("dist_threshold", C.c_float), ("angle_threshold_deg", C.c_float),
                ("height_threshold", C.c_float), ("cos_normal_threshold", C.c_float), ("min_planes_recognition", C.c_int),
                ("max_curvature_plane", C.c_float), ("min_area_plane", C.c_float), ("max_elongation_plane", C.c_float),
                ("up_axis", C.c_int), ("planar_normal_tol", C.c_float), ("max_conditioning", C.c_float),
                ("sigma_dist", C.c_float), ("sigma_normal", C.c_float), ("max_nodes", C.c_int),
                ("use_color", C.c_int), ("color_threshold", C.c_float), ("intensity_threshold", C.c_float), ("hue_threshold", C.c_float)]


_lib = None


def load() -> C.CDLL:
    """Returns the loaded HIP library or raises; never substitutes another implementation."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(rgbd360_amd has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, i32, f32p = C.c_void_p, C.c_int, C.c_void_p
    L.rgbd360_default_params.argtypes = [C.POINTER(Params)]
    L.rgbd360_default_params.restype = None
    L.rgbd360_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.rgbd360_destroy.argtypes = [vp]
    L.rgbd360_destroy.restype = None
    L.rgbd360_last_error.argtypes = [vp]
    L.rgbd360_last_error.restype = C.c_char_p
    for f in (L.rgbd360_set_target, L.rgbd360_set_source, L.rgbd360_set_target_dev, L.rgbd360_set_source_dev):
        f.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32]
    L.rgbd360_promote_source_to_target.argtypes = [vp]
    L.rgbd360_align360.argtypes = [vp, f32p, i32, i32, f32p, C.POINTER(Result)]
    L.rgbd360_align360_begin.argtypes = [vp, f32p, i32, i32]
    L.rgbd360_align360_finish.argtypes = [vp, f32p, C.POINTER(Result)]
    L.rgbd360_align360_batch.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, f32p, i32, i32, i32, f32p, vp]
    L.rgbd360_align360_batch_dev.argtypes = L.rgbd360_align360_batch.argtypes
    L.rgbd360_level_dims.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.rgbd360_get_plane.argtypes = [vp, i32, i32, f32p]
    L.rgbd360_get_lut.argtypes = [vp, i32, f32p]
    L.rgbd360_eval.argtypes = [vp, i32, f32p, i32, C.POINTER(C.c_double), C.POINTER(C.c_longlong), vp, vp, vp, vp, vp, vp,
                               C.POINTER(C.c_longlong)]
    L.rgbd360_eval_occ.argtypes = [vp, i32, f32p, i32, i32, C.POINTER(C.c_double), C.POINTER(C.c_longlong), vp, vp, vp, vp, vp, vp,
                                   C.POINTER(C.c_longlong)]
    L.rgbd360_warp_indices.argtypes = [vp, i32, f32p, vp]
    L.rgbd360_set_camera.argtypes = [vp, C.c_float, C.c_float, C.c_float, C.c_float]
    L.rgbd360_align_pinhole.argtypes = [vp, f32p, i32, i32, f32p, C.POINTER(Result)]
    L.rgbd360_eval_pinhole.argtypes = [vp, i32, f32p, i32, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_longlong)]
    L.rgbd360_eval_pinhole_occ.argtypes = [vp, i32, f32p, i32, i32, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_longlong)]
    L.rgbd360_use_saliency.argtypes = [vp, i32, C.c_float]
    L.rgbd360_warp_indices_pinhole.argtypes = [vp, i32, f32p, vp]
    for f in (L.rgbd360_warp_images, L.rgbd360_warp_images_dev, L.rgbd360_warp_images_pinhole):
        f.argtypes = [vp, i32, f32p, i32, vp, vp, vp, vp, vp]
    L.rgbd360_time_warp_images.argtypes = [vp, i32, f32p, i32, i32, vp]
    L.rgbd360_gn_step.argtypes = [vp, f32p, f32p, C.c_float, f32p, f32p, f32p]
    L.rgbd360_forced_iters.argtypes = [vp, i32, f32p, i32, i32, f32p, C.POINTER(C.c_double), C.POINTER(C.c_float)]
    L.rgbd360_time_eval_kernel.argtypes = [vp, i32, f32p, i32, i32, i32, C.POINTER(C.c_float)]
    L.rgbd360_stream.argtypes = [vp]
    L.rgbd360_stream.restype = vp
    L.rgbd360_sync.argtypes = [vp]
    L.rgbd360_device_count.argtypes = []
    L.rgbd360_time_solve_kernel.argtypes = [vp, i32, i32, i32, C.POINTER(C.c_float)]
    L.rgbd360_normals.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float, i32, vp]
    L.rgbd360_distance_map.argtypes = [vp, vp, i32, i32, C.c_float, i32, vp]
    L.rgbd360_bilateral_filter.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float, vp]
    L.rgbd360_sensor_cloud.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, C.c_float, C.c_float, vp]
    L.rgbd360_sensor_planes.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i32,
                                        C.c_float, C.c_float, C.c_float, vp, vp, i32, C.POINTER(i32)]
    L.rgbd360_merge_planes.argtypes = [vp, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32, C.POINTER(i32)]
    L.rgbd360_sensor_cloud_ex.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, C.c_float, C.c_float, vp]
    L.rgbd360_sensor_planes_ex.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, i32,
                                           C.c_float, C.c_float, C.c_float, vp, vp, i32, C.POINTER(i32)]
    L.rgbd360_depth_model_load.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.rgbd360_depth_model_free.argtypes = [vp]
    L.rgbd360_depth_model_free.restype = None
    L.rgbd360_depth_model_info.argtypes = [vp, C.POINTER(i32), C.POINTER(C.c_double)]
    L.rgbd360_depth_model_undistort.argtypes = [vp, vp, C.c_size_t, i32, i32]
    L.rgbd360_depth_model_from_sums.argtypes = [i32, i32, i32, i32, C.c_double, i32, vp, vp, vp, C.POINTER(vp)]
    L.rgbd360_depth_model_save.argtypes = [vp, C.c_char_p]
    L.rgbd360_depth_trainer_create.argtypes = [vp, i32, i32, i32, i32, C.c_double, i32, C.POINTER(vp)]
    L.rgbd360_depth_trainer_destroy.argtypes = [vp]
    L.rgbd360_depth_trainer_destroy.restype = None
    L.rgbd360_depth_trainer_last_error.argtypes = [vp]
    L.rgbd360_depth_trainer_last_error.restype = C.c_char_p
    L.rgbd360_depth_trainer_clear.argtypes = [vp]
    L.rgbd360_depth_default_train_params.argtypes = [vp, C.POINTER(DepthTrainParams)]
    L.rgbd360_depth_default_train_params.restype = None
    L.rgbd360_depth_trainer_accumulate_images.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, C.POINTER(DepthTrainParams),
                                                          C.POINTER(DepthTrainStats)]
    L.rgbd360_depth_trainer_accumulate_map.argtypes = [vp, vp, vp, C.c_size_t, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, f32p, i32,
                                                       C.POINTER(DepthTrainParams), vp, C.POINTER(DepthTrainStats)]
    L.rgbd360_depth_trainer_sums.argtypes = [vp, vp, vp, vp]
    L.rgbd360_depth_trainer_add_sums.argtypes = [vp, vp, vp, vp]
    L.rgbd360_depth_trainer_model.argtypes = [vp, C.POINTER(vp)]
    L.rgbd360_depth_trainer_set_form.argtypes = [vp, i32]
    L.rgbd360_depth_models_create.argtypes = [vp, C.POINTER(vp), i32, C.POINTER(vp)]
    L.rgbd360_depth_models_destroy.argtypes = [vp]
    L.rgbd360_depth_models_destroy.restype = None
    L.rgbd360_depth_models_bytes.argtypes = [vp]
    L.rgbd360_depth_models_bytes.restype = C.c_size_t
    L.rgbd360_depth_models_set.argtypes = [vp, i32, vp]
    L.rgbd360_depth_undistort.argtypes = [vp, vp, C.POINTER(MapBatchFrame), C.POINTER(i32), i32, i32, i32, i32, i32, C.POINTER(vp), C.c_size_t]
    L.rgbd360_rig_depth_clouds.argtypes = [vp, vp, C.POINTER(MapBatchFrame), i32, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, i32, vp]
    L.rgbd360_depth_evaluate_map.argtypes = [vp, vp, vp, i32, vp, C.c_size_t, i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, f32p, i32,
                                             C.POINTER(DepthTrainParams), C.POINTER(DepthTrainStats), C.POINTER(DepthEvalSums)]
    L.rgbd360_depth_models_pack.argtypes = [C.POINTER(vp), i32, vp, C.POINTER(C.c_size_t)]
    L.rgbd360_depth_models_repack.argtypes = [vp, i32, vp, vp, C.POINTER(C.c_size_t)]
    L.rgbd360_depth_models_undistort_packed_host.argtypes = [vp, i32, vp, C.c_size_t, i32, i32]
    L.rgbd360_depth_apply_timing.argtypes = [vp, i32]
    L.rgbd360_depth_apply_last_us.argtypes = [vp, C.POINTER(C.c_float)]
    L.rgbd360_depth_apply_time_copy.argtypes = [vp, vp, vp, C.c_size_t, C.POINTER(C.c_float)]
    L.rgbd360_depth_trainer_time_map.argtypes = [vp, vp, vp, C.c_size_t, i32, C.c_float, C.c_float, C.c_float, C.c_float, f32p,
                                                 C.POINTER(DepthTrainParams), vp, vp, i32, vp, vp, C.POINTER(DepthTrainStats)]
    L.rgbd360_pool_sensor_planes.argtypes = [vp, i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32, C.POINTER(i32)]
    L.rgbd360_pool_sensor_planes.restype = i32
    L.rgbd360_debug_set_schedule.argtypes = [vp, i32, i32]
    L.rgbd360_debug_set_sequence_route.argtypes = [vp, i32, i32]
    L.rgbd360_debug_knobs_enabled.argtypes = []
    L.rgbd360_frame_planes_stage_timing.argtypes = [vp, i32]
    L.rgbd360_frame_planes_stage_times.argtypes = [vp, C.POINTER(C.c_float)]
    L.rgbd360_group_planes.argtypes = [vp, C.POINTER(i32), i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, vp, i32, C.POINTER(i32)]
    L.rgbd360_cloud_planes.argtypes = [vp, vp, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float, i32, C.c_float, C.c_float, C.c_float, i32, vp,
                                       vp, i32, C.POINTER(i32)]
    L.rgbd360_plane_fit.argtypes = [vp, vp, vp, i32, i32, i32, C.c_float, C.c_float, C.c_float, i32, vp, vp, i32, C.POINTER(i32)]
    L.rgbd360_frame_planes.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, C.c_float, C.c_float, i32, C.c_float, C.c_float, C.c_float,
                                       i32, vp, vp, vp, vp, i32, C.POINTER(i32)]
    L.rgbd360_frame_planes_dev.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, C.c_float, C.c_float, i32, C.c_float, C.c_float,
                                           C.c_float, i32, vp, i32, C.POINTER(i32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.rgbd360_load_frame_bin.argtypes = [C.c_char_p, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.rgbd360_stitch_sphere.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp, vp, C.POINTER(i32), C.POINTER(i32)]
    L.rgbd360_selftest_math.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.rgbd360_selftest_libm.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.rgbd360_set_index_arithmetic.argtypes = [vp, C.c_int]
    L.rgbd360_get_index_arithmetic.argtypes = [vp]
    L.rgbd360_sphere_cloud.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p]
    L.rgbd360_pbmap_default_params.argtypes = [C.POINTER(PbmapParams), i32]
    L.rgbd360_pbmap_default_params.restype = None
    L.rgbd360_register_planes.argtypes = [vp, i32, vp, i32, i32, i32, C.POINTER(PbmapParams), vp, vp, vp, C.POINTER(i32),
                                          C.POINTER(C.c_float)]
    L.rgbd360_planes_available.argtypes = [vp]
    L.rgbd360_forced_iters_batch.argtypes = [vp, i32, vp, vp, vp, vp, C.c_size_t, C.c_size_t, i32, i32, i32, i32, f32p, i32, i32, f32p,
                                             C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.rgbd360_debug_solve_partials.argtypes = [vp, i32, vp, i32, i32, vp, f32p, f32p]
    L.rgbd360_debug_solve_state.argtypes = [vp, i32, vp, C.POINTER(SolveStateIn), i32, i32, i32, C.POINTER(SolveStateOut)]
    L.rgbd360_debug_solve_table.argtypes = [vp, i32, vp, i32, i32, i32, i32, vp, vp, f32p]
    L.rgbd360_set_plane_refinement.argtypes = [vp, i32, C.c_float]
    L.rgbd360_set_plane_color_image.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32]
    L.rgbd360_plane_refinement_stats.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.rgbd360_debug_plane_sums.argtypes = [vp, i32, C.POINTER(i32), vp, vp, vp]
    L.rgbd360_rig_create.argtypes = [C.POINTER(Params), i32, vp, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(vp)]
    L.rgbd360_rig_destroy.argtypes = [vp]
    L.rgbd360_rig_destroy.restype = None
    L.rgbd360_rig_last_error.argtypes = [vp]
    L.rgbd360_rig_last_error.restype = C.c_char_p
    for f in (L.rgbd360_rig_set_target, L.rgbd360_rig_set_source):
        f.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32]
    L.rgbd360_rig_eval.argtypes = [vp, i32, f32p, i32, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_longlong)]
    L.rgbd360_rig_align.argtypes = [vp, f32p, i32, f32p, C.POINTER(Result)]
    L.rgbd360_rig_use_saliency.argtypes = [vp, i32, C.c_float]
    L.rgbd360_rig_set_index_arithmetic.argtypes = [vp, C.c_int]
    L.rgbd360_rig_get_index_arithmetic.argtypes = [vp]
    L.rgbd360_rig_warp_indices.argtypes = [vp, i32, f32p, i32, vp]
    L.rgbd360_time_eval_kernel_rotating.argtypes = [vp, i32, i32, f32p, i32, i32, i32, C.POINTER(C.c_float)]
    L.rgbd360_multi_create.argtypes = [C.POINTER(Params), i32, vp, C.POINTER(vp)]
    L.rgbd360_multi_destroy.argtypes = [vp]
    L.rgbd360_multi_destroy.restype = None
    L.rgbd360_multi_last_error.argtypes = [vp]
    L.rgbd360_multi_last_error.restype = C.c_char_p
    L.rgbd360_multi_n_gpus.argtypes = [vp]
    L.rgbd360_multi_uses_rccl.argtypes = [vp]
    L.rgbd360_multi_set_index_arithmetic.argtypes = [vp, C.c_int]
    L.rgbd360_shard_range.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.rgbd360_shard_range.restype = None
    L.rgbd360_gather_slot.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.rgbd360_gather_slot.restype = None
    L.rgbd360_multi_align_sequence.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, f32p, i32, i32, i32, f32p, vp]
    L.rgbd360_multi_load_sequence.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32]
    L.rgbd360_multi_align_resident.argtypes = [vp, f32p, i32, i32, i32, f32p, vp]
    L.rgbd360_align360_batch_multi.argtypes = [C.POINTER(Params), i32, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, f32p, i32, i32, i32,
                                               i32, vp, f32p, vp]
    L.rgbd360_store_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.rgbd360_store_destroy.argtypes = [vp]
    L.rgbd360_store_destroy.restype = None
    L.rgbd360_store_last_error.argtypes = [vp]
    L.rgbd360_store_last_error.restype = C.c_char_p
    L.rgbd360_store_entry_bytes.argtypes = [vp]
    L.rgbd360_store_entry_bytes.restype = C.c_size_t
    L.rgbd360_store_put.argtypes = [vp, i32, vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32]
    L.rgbd360_store_occupied.argtypes = [vp, i32]
    L.rgbd360_store_align.argtypes = [vp, i32, vp, vp, f32p, i32, i32, i32, f32p, vp]
    L.rgbd360_store_overlap_default_params.argtypes = [vp, C.POINTER(OverlapParams)]
    L.rgbd360_store_overlap_default_params.restype = None
    L.rgbd360_store_overlap.argtypes = [vp, i32, vp, vp, f32p, C.POINTER(OverlapParams), vp]
    L.rgbd360_store_overlap_all.argtypes = [vp, i32, vp, f32p, C.c_float, C.POINTER(OverlapParams), vp, f32p]
    L.rgbd360_overlap_candidates.argtypes = [i32, vp, i32, C.c_float, i32, i32, i32, vp, vp, i32, vp, vp, vp]
    L.rgbd360_overlap_representative.argtypes = [i32, vp, i32, vp, i32]
    L.rgbd360_store_time_overlap.argtypes = [vp, i32, vp, vp, f32p, C.POINTER(OverlapParams), i32, vp, vp]
    L.rgbd360_store_time_overlap_all.argtypes = [vp, i32, vp, f32p, C.c_float, C.POINTER(OverlapParams), i32, i32, vp, vp]
    ll = C.c_longlong
    L.rgbd360_map_create.argtypes = [vp, C.c_float, ll, C.POINTER(vp)]
    L.rgbd360_map_destroy.argtypes = [vp]
    L.rgbd360_map_destroy.restype = None
    L.rgbd360_map_last_error.argtypes = [vp]
    L.rgbd360_map_last_error.restype = C.c_char_p
    L.rgbd360_map_bytes.argtypes = [vp]
    L.rgbd360_map_bytes.restype = C.c_size_t
    L.rgbd360_map_set_box.argtypes = [vp, vp, vp]
    L.rgbd360_map_insert_sphere.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapStats)]
    L.rgbd360_map_insert_cloud.argtypes = [vp, vp, vp, ll, f32p, i32, C.POINTER(MapStats)]
    L.rgbd360_map_size.argtypes = [vp]
    L.rgbd360_map_size.restype = ll
    L.rgbd360_map_clear.argtypes = [vp]
    for f in (L.rgbd360_map_extract, L.rgbd360_map_extract_dev):
        f.argtypes = [vp, ll, vp, vp, vp, vp]
        f.restype = ll
    L.rgbd360_map_time_kernels.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, vp, C.POINTER(ll)]
    L.rgbd360_map_remove_sphere.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapEditStats)]
    L.rgbd360_map_remove_cloud.argtypes = [vp, vp, vp, ll, f32p, i32, C.POINTER(MapEditStats)]
    L.rgbd360_map_move_sphere.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, f32p, i32, C.POINTER(MapEditStats),
                                          C.POINTER(MapStats)]
    L.rgbd360_map_move_cloud.argtypes = [vp, vp, vp, ll, f32p, f32p, i32, C.POINTER(MapEditStats), C.POINTER(MapStats)]
    L.rgbd360_map_rehash.argtypes = [vp, ll]
    L.rgbd360_map_census.argtypes = [vp, C.POINTER(MapCensus)]
    L.rgbd360_map_time_edit.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, vp]
    L.rgbd360_map_default_align_params.argtypes = [vp, C.POINTER(MapAlignParams)]
    L.rgbd360_map_default_align_params.restype = None
    L.rgbd360_map_align_sphere.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapAlignParams), f32p, C.POINTER(MapAlignResult)]
    L.rgbd360_map_align_cloud.argtypes = [vp, vp, ll, f32p, i32, C.POINTER(MapAlignParams), f32p, C.POINTER(MapAlignResult)]
    L.rgbd360_map_align_eval.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, vp, ll, f32p, i32, C.POINTER(MapAlignParams), vp, vp, vp, vp, i32,
                                         C.POINTER(i32), vp]
    L.rgbd360_map_time_align.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, C.POINTER(MapAlignParams), i32, vp, C.POINTER(C.c_double)]
    L.rgbd360_map_default_align_plane_params.argtypes = [vp, C.POINTER(MapAlignPlaneParams)]
    L.rgbd360_map_default_align_plane_params.restype = None
    L.rgbd360_map_align_plane_sphere.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapAlignPlaneParams), f32p,
                                                 C.POINTER(MapAlignPlaneResult)]
    L.rgbd360_map_align_plane_cloud.argtypes = [vp, vp, ll, f32p, i32, C.POINTER(MapAlignPlaneParams), f32p, C.POINTER(MapAlignPlaneResult)]
    for name, pt, rt in (("rgbd360_map_align", MapAlignParams, MapAlignResult), ("rgbd360_map_align_plane", MapAlignPlaneParams, MapAlignPlaneResult)):
        getattr(L, name + "_batch_cloud").argtypes = [vp, C.POINTER(MapBatchCloud), i32, i32, C.POINTER(MapBatchJob), i32, C.POINTER(pt), vp, C.POINTER(rt)]
        getattr(L, name + "_batch_sphere").argtypes = [vp, C.POINTER(MapBatchFrame), i32, i32, i32, i32, i32, i32, C.POINTER(MapBatchJob), i32, C.POINTER(pt), vp,
                                                       C.POINTER(rt)]
        getattr(L, name + "_best").argtypes = [C.POINTER(rt), i32, ll]
    L.rgbd360_map_align_batch_trace.argtypes = [vp, i32, i32, C.POINTER(i32), C.POINTER(MapAlignTrace)]
    L.rgbd360_map_default_rig_calib_params.argtypes = [vp, C.POINTER(RigCalibParams)]
    L.rgbd360_map_default_rig_calib_params.restype = None
    rig_tail = [i32, i32, i32, vp, vp, C.POINTER(RigCalibParams), C.POINTER(RigCalibResult), C.POINTER(RigCalibSensor)]
    L.rgbd360_map_calibrate_rig_clouds.argtypes = [vp, C.POINTER(MapBatchCloud)] + rig_tail
    L.rgbd360_map_calibrate_rig_depth.argtypes = [vp, C.POINTER(MapBatchFrame), i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float] + rig_tail
    L.rgbd360_map_calibrate_rig_depth_models.argtypes = [vp, vp, C.POINTER(MapBatchFrame), i32, i32, i32, C.c_float, C.c_float, C.c_float, C.c_float] + rig_tail
    L.rgbd360_rig_save_extrinsics.argtypes = [vp, i32, C.c_char_p]
    L.rgbd360_rig_calib_solve_host.argtypes = [vp, i32, i32, vp, vp, C.POINTER(RigCalibParams), vp, vp, vp, C.POINTER(i32)]
    L.rgbd360_rig_calib_solve_dev.argtypes = [vp] + L.rgbd360_rig_calib_solve_host.argtypes
    L.rgbd360_rig_calib_trace.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(RigCalibStep)]
    L.rgbd360_rig_calib_time_solve.argtypes = [vp, vp, i32, i32, vp, vp, C.POINTER(RigCalibParams), i32, vp]
    L.rgbd360_map_align_plane_eval.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, vp, ll, f32p, i32, C.POINTER(MapAlignPlaneParams), vp, vp, vp, vp,
                                               vp, vp]
    L.rgbd360_map_plane_fit.argtypes = [vp, C.c_double, vp, vp]
    L.rgbd360_map_time_align_plane.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, C.POINTER(MapAlignPlaneParams), i32, vp,
                                               C.POINTER(C.c_double)]
    L.rgbd360_map_default_align_gicp_params.argtypes = [vp, C.POINTER(MapAlignGicpParams)]
    L.rgbd360_map_default_align_gicp_params.restype = None
    L.rgbd360_map_align_gicp_sphere.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapAlignGicpParams), f32p,
                                                C.POINTER(MapAlignGicpResult)]
    L.rgbd360_map_align_gicp_cloud.argtypes = [vp, vp, vp, ll, f32p, i32, C.POINTER(MapAlignGicpParams), f32p, C.POINTER(MapAlignGicpResult)]
    L.rgbd360_map_align_gicp_eval.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, vp, vp, ll, f32p, i32, C.POINTER(MapAlignGicpParams), vp, vp, vp,
                                              vp, vp, vp]
    L.rgbd360_map_gicp_weight.argtypes = [vp, i32, vp, i32, vp, C.c_float, vp]
    L.rgbd360_map_time_align_gicp.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, C.POINTER(MapAlignGicpParams), i32, vp,
                                              C.POINTER(C.c_double)]
    L.rgbd360_map_default_render_params.argtypes = [vp, C.POINTER(MapRenderParams)]
    L.rgbd360_map_default_render_params.restype = None
    L.rgbd360_map_render_sphere.argtypes = [vp, i32, i32, f32p, C.POINTER(MapRenderParams), vp, vp, vp, vp, C.POINTER(MapRenderStats)]
    L.rgbd360_map_render_sphere_dev.argtypes = [vp, i32, i32, f32p, C.POINTER(MapRenderParams), vp, vp, vp, vp, vp]
    L.rgbd360_map_time_render.argtypes = [vp, i32, i32, f32p, C.POINTER(MapRenderParams), i32, i32, vp, C.POINTER(MapRenderStats), C.POINTER(ll)]
    L.rgbd360_map_default_raycast_params.argtypes = [vp, C.POINTER(MapRaycastParams)]
    L.rgbd360_map_default_raycast_params.restype = None
    L.rgbd360_map_raycast.argtypes = [vp, ll, vp, vp, i32, C.POINTER(MapRaycastParams), vp, vp, vp, vp, vp, C.POINTER(MapRaycastStats)]
    L.rgbd360_map_raycast_sphere.argtypes = [vp, i32, i32, f32p, C.POINTER(MapRaycastParams), vp, vp, vp, vp, C.POINTER(MapRaycastStats)]
    L.rgbd360_map_raycast_sphere_dev.argtypes = [vp, i32, i32, f32p, C.POINTER(MapRaycastParams), vp, vp, vp, vp, vp]
    L.rgbd360_map_raycast_set_plain.argtypes = [vp, i32]
    L.rgbd360_map_time_raycast.argtypes = [vp, ll, vp, vp, i32, i32, f32p, C.POINTER(MapRaycastParams), i32, i32, vp, vp, vp, C.POINTER(MapRaycastStats),
                                           C.POINTER(ll)]
    L.rgbd360_map_default_colour_params.argtypes = [vp, C.POINTER(MapColourParams)]
    L.rgbd360_map_default_colour_params.restype = None
    L.rgbd360_map_colours.argtypes = [vp, C.POINTER(MapColourParams), ll, vp, vp, vp, vp, vp, vp, C.POINTER(MapColourStats)]
    L.rgbd360_map_colours.restype = ll
    L.rgbd360_map_colours_dev.argtypes = [vp, C.POINTER(MapColourParams), ll, vp, vp, vp, vp, vp, vp, vp]
    L.rgbd360_map_colours_dev.restype = ll
    L.rgbd360_map_colour_bytes.argtypes = [vp]
    L.rgbd360_map_colour_bytes.restype = C.c_size_t
    L.rgbd360_map_release_colours.argtypes = [vp]
    L.rgbd360_map_colour_gradient.argtypes = [vp, C.c_float, i32, vp, vp, i32, C.c_float, vp]
    L.rgbd360_map_colour_intensity.argtypes = [ll, ll, ll, ll]
    L.rgbd360_map_colour_intensity.restype = C.c_double
    L.rgbd360_map_time_colours.argtypes = [vp, C.POINTER(MapColourParams), i32, vp, vp, vp, C.POINTER(MapColourStats), C.POINTER(ll)]
    L.rgbd360_map_default_align_colour_params.argtypes = [vp, C.POINTER(MapAlignColourParams)]
    L.rgbd360_map_default_align_colour_params.restype = None
    L.rgbd360_map_align_colour_sphere.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapAlignColourParams), f32p,
                                                  C.POINTER(MapAlignColourResult)]
    L.rgbd360_map_align_colour_cloud.argtypes = [vp, vp, vp, ll, f32p, i32, C.POINTER(MapAlignColourParams), f32p, C.POINTER(MapAlignColourResult)]
    L.rgbd360_map_align_colour_eval.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, vp, vp, ll, f32p, i32,
                                                C.POINTER(MapAlignColourParams), vp, vp, vp, vp, vp, vp]
    L.rgbd360_map_time_align_colour.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, C.POINTER(MapAlignColourParams), i32, vp,
                                                C.POINTER(C.c_double)]
    L.rgbd360_map_set_align_robust.argtypes = [vp, i32, C.POINTER(MapRobust)]
    L.rgbd360_map_get_align_robust.argtypes = [vp, i32, C.POINTER(MapRobust)]
    L.rgbd360_map_align_robust_info.argtypes = [vp, C.POINTER(MapRobustInfo)]
    L.rgbd360_map_align_batch_robust_info.argtypes = [vp, i32, C.POINTER(MapRobustInfo)]
    L.rgbd360_map_align_robust_eval.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, vp, vp, vp, ll, f32p, i32, vp, vp, vp]
    L.rgbd360_map_time_align_robust.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t, i32, i32, i32, i32, f32p, vp, i32, vp]
    L.rgbd360_map_default_normal_params.argtypes = [vp, C.POINTER(MapNormalParams)]
    L.rgbd360_map_default_normal_params.restype = None
    L.rgbd360_map_normals.argtypes = [vp, C.POINTER(MapNormalParams), vp, ll, vp, vp, vp, vp, vp, vp, C.POINTER(MapNormalStats)]
    L.rgbd360_map_normals.restype = ll
    L.rgbd360_map_normals_dev.argtypes = [vp, C.POINTER(MapNormalParams), vp, ll, vp, vp, vp, vp, vp, vp, vp]
    L.rgbd360_map_normals_dev.restype = ll
    L.rgbd360_map_raycast_surface.argtypes = [vp, ll, vp, vp, i32, C.POINTER(MapRaycastParams), C.POINTER(MapNormalParams), vp, vp, vp, vp, vp, vp,
                                              C.POINTER(ll), C.POINTER(MapRaycastStats)]
    L.rgbd360_map_raycast_surface_sphere.argtypes = [vp, i32, i32, f32p, C.POINTER(MapRaycastParams), C.POINTER(MapNormalParams), vp, vp, vp, vp, vp,
                                                     C.POINTER(ll), C.POINTER(MapRaycastStats)]
    L.rgbd360_map_raycast_surface_sphere_dev.argtypes = [vp, i32, i32, f32p, C.POINTER(MapRaycastParams), C.POINTER(MapNormalParams), vp, vp, vp, vp, vp,
                                                         vp, vp]
    L.rgbd360_map_time_normals.argtypes = [vp, C.POINTER(MapNormalParams), i32, vp, vp, C.POINTER(MapNormalStats), C.POINTER(ll)]
    L.rgbd360_map_default_observe_params.argtypes = [vp, C.POINTER(MapObserveParams)]
    L.rgbd360_map_default_observe_params.restype = None
    L.rgbd360_map_observe_sphere.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapObserveParams), C.POINTER(MapObserveStats)]
    L.rgbd360_map_observe_rays.argtypes = [vp, ll, vp, vp, i32, C.POINTER(MapObserveParams), C.POINTER(MapObserveStats)]
    L.rgbd360_map_votes.argtypes = [vp, ll, vp, vp, vp, vp]
    L.rgbd360_map_votes.restype = ll
    L.rgbd360_map_carve.argtypes = [vp, i32, i32, i32, C.POINTER(MapCarveStats)]
    L.rgbd360_map_vote_bytes.argtypes = [vp]
    L.rgbd360_map_vote_bytes.restype = C.c_size_t
    L.rgbd360_map_release_votes.argtypes = [vp]
    L.rgbd360_map_time_observe.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, C.POINTER(MapObserveParams), i32, i32, vp, vp,
                                           C.POINTER(MapObserveStats)]
    L.rgbd360_map_default_plane_seg_params.argtypes = [vp, C.POINTER(MapPlaneSegParams)]
    L.rgbd360_map_default_plane_seg_params.restype = None
    L.rgbd360_map_planes.argtypes = [vp, C.POINTER(MapPlaneSegParams), vp, i32, vp, vp, C.POINTER(i32), C.POINTER(MapPlaneSegStats)]
    L.rgbd360_map_plane_labels.argtypes = [vp, C.POINTER(MapPlaneSegParams), ll, vp, vp, vp]
    L.rgbd360_map_plane_labels.restype = ll
    L.rgbd360_map_plane_bytes.argtypes = [vp]
    L.rgbd360_map_plane_bytes.restype = C.c_size_t
    L.rgbd360_map_release_planes.argtypes = [vp]
    L.rgbd360_map_plane_from_sums.argtypes = [ll, ll, vp, vp, vp, C.POINTER(Plane)]
    L.rgbd360_map_plane_from_members.argtypes = [ll, ll, vp, vp, vp, vp, vp, C.POINTER(Plane)]
    L.rgbd360_map_plane_sums_in_range.argtypes = [ll, ll, C.c_float]
    L.rgbd360_map_time_planes.argtypes = [vp, C.POINTER(MapPlaneSegParams), i32, i32, vp, C.POINTER(MapPlaneSegStats)]
    L.rgbd360_map_level.argtypes = [vp, i32, C.POINTER(vp)]
    L.rgbd360_map_pyramid_bytes.argtypes = [vp]
    L.rgbd360_map_pyramid_bytes.restype = C.c_size_t
    L.rgbd360_map_release_levels.argtypes = [vp]
    L.rgbd360_map_default_c2f_params.argtypes = [vp, C.POINTER(MapC2fParams)]
    L.rgbd360_map_default_c2f_params.restype = None
    L.rgbd360_map_align_c2f_sphere.argtypes = [vp, vp, C.c_size_t, i32, i32, i32, i32, f32p, i32, C.POINTER(MapC2fParams), f32p, C.POINTER(MapC2fResult)]
    L.rgbd360_map_align_c2f_cloud.argtypes = [vp, vp, ll, f32p, i32, C.POINTER(MapC2fParams), f32p, C.POINTER(MapC2fResult)]
    L.rgbd360_map_time_coarsen.argtypes = [vp, i32, i32, vp, vp]
    L.rgbd360_map_default_merge_params.argtypes = [vp, C.POINTER(MapMergeParams)]
    L.rgbd360_map_default_merge_params.restype = None
    for f in (L.rgbd360_map_merge, L.rgbd360_map_unmerge):
        f.argtypes = [vp, vp, f32p, C.POINTER(MapMergeParams), C.POINTER(MapMergeStats)]
    L.rgbd360_map_records.argtypes = [vp, ll, vp]
    L.rgbd360_map_records.restype = ll
    L.rgbd360_map_add_records.argtypes = [vp, vp, ll, i32, C.POINTER(MapMergeStats)]
    L.rgbd360_map_time_merge.argtypes = [vp, vp, f32p, i32, vp]
    L.rgbd360_graph_create.argtypes = [vp, C.POINTER(vp)]
    L.rgbd360_graph_destroy.argtypes = [vp]
    L.rgbd360_graph_destroy.restype = None
    L.rgbd360_graph_last_error.argtypes = [vp]
    L.rgbd360_graph_last_error.restype = C.c_char_p
    L.rgbd360_graph_add_vertices.argtypes = [vp, i32, f32p, vp]
    L.rgbd360_graph_add_edges.argtypes = [vp, i32, vp, vp, f32p, f32p]
    L.rgbd360_graph_set_poses.argtypes = [vp, i32, i32, f32p]
    L.rgbd360_graph_set_fixed.argtypes = [vp, i32, i32, vp]
    L.rgbd360_graph_n_vertices.argtypes = [vp]
    L.rgbd360_graph_n_edges.argtypes = [vp]
    L.rgbd360_graph_clear.argtypes = [vp]
    L.rgbd360_graph_default_params.argtypes = [C.POINTER(GraphParams)]
    L.rgbd360_graph_default_params.restype = None
    L.rgbd360_graph_optimize.argtypes = [vp, C.POINTER(GraphParams), C.POINTER(GraphResult)]
    L.rgbd360_graph_get_poses.argtypes = [vp, i32, i32, f32p]
    L.rgbd360_graph_chi2.argtypes = [vp, C.POINTER(C.c_double), vp]
    L.rgbd360_graph_get_trace.argtypes = [vp, i32, C.POINTER(i32), vp]
    L.rgbd360_graph_linearize.argtypes = [vp, vp, vp]
    L.rgbd360_graph_apply.argtypes = [vp, C.c_double, vp, vp]
    L.rgbd360_graph_time_kernels.argtypes = [vp, i32, vp]
    L.rgbd360_graph_set_edge_robust.argtypes = [vp, i32, i32, vp, vp]
    L.rgbd360_graph_set_edge_enabled.argtypes = [vp, i32, i32, vp]
    L.rgbd360_graph_get_edge_state.argtypes = [vp, i32, i32, vp, vp, vp]
    L.rgbd360_graph_edge_weights.argtypes = [vp, C.POINTER(C.c_double), vp, vp, vp]
    L.rgbd360_graph_default_cov_params.argtypes = [C.POINTER(GraphCovParams)]
    L.rgbd360_graph_default_cov_params.restype = None
    L.rgbd360_graph_marginals.argtypes = [vp, i32, vp, C.POINTER(GraphCovParams), vp, vp, vp, C.POINTER(GraphCovResult)]
    L.rgbd360_graph_relative_covariances.argtypes = [vp, i32, vp, vp, C.POINTER(GraphCovParams), vp, vp, vp, C.POINTER(GraphCovResult)]
    L.rgbd360_graph_time_cov_kernels.argtypes = [vp, i32, vp, i32, vp]
    _lib = L
    return L
