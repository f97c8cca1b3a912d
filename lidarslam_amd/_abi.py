"""The C ABI of liblidarslam_amd.so as ctypes sees it: one table of signatures, applied once when the library loads.

SIGNATURES has an entry ``name: (restype, [argtypes])`` for every function include/lidarslam_amd.h declares, in the
header's order.  Handles and buffers are ``c_void_p`` (so ``byref(...)``, ctypes arrays, ``None`` and ``ptr(array)`` all
pass), strings ``c_char_p``, a ``void`` result is ``None``.  No other file of the package assigns ``.argtypes`` or
``.restype``; tests/test_abi.py holds every entry to the header's prototype.
"""
import ctypes as C
import os

from ._native import LIB_PATH, ExtractParams, MatchParams


class LsaError(RuntimeError):
    code = None  # the LSA_E_* value of the call that failed, where there was one


E_NO_DEVICE, E_HIP, E_ARG, E_STATE, E_CAPACITY = -1, -2, -3, -4, -5
TARGET_MAP, TARGET_PREVIOUS = 0, 1
KNN_MAX = 16  # LSA_KNN_MAX: slots per query of the neighbour lists (Context.knn_lists)


def _error(what, rc, message):
    e = LsaError(f"{what} failed ({rc}): {message}")
    e.code = rc
    return e


class IcpLink(C.Structure):
    """lsa_icp_link_t (include/lidarslam_amd.h): what a solve needs to prepare the ICP iteration enqueued behind it."""

    _fields_ = [
        ("refine_undistortion", C.c_int), ("first", C.c_int), ("have_log", C.c_int),
        ("prev_time", C.c_double), ("cur_time", C.c_double), ("max_extrapolation_ratio", C.c_double),
        ("previous_world", C.c_double * 16), ("motion", C.c_double * 16),
    ]


class SolveResult(C.Structure):
    """lsa_solve_result_t (include/lidarslam_amd.h)."""

    _fields_ = [
        ("pose", C.c_double * 6), ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("cost", C.c_double), ("g", C.c_double * 6), ("H", C.c_double * 36),
        ("num_successful_steps", C.c_int), ("num_unsuccessful_steps", C.c_int), ("num_iterations", C.c_int),
        ("num_evaluations", C.c_int), ("num_matches", C.c_int), ("skipped", C.c_int), ("termination", C.c_int),
        ("message", C.c_char_p),
    ]


vp, s, i32, u32, f32, f64 = C.c_void_p, C.c_char_p, C.c_int, C.c_uint, C.c_float, C.c_double
u64, i64, ull, sz, P = C.c_uint64, C.c_longlong, C.c_ulonglong, C.c_size_t, C.POINTER

SIGNATURES = {
    # ---- context, frames, extraction
    "lsa_device_count": (i32, []),
    "lsa_ctx_create": (i32, [i32, P(vp)]),
    "lsa_bind_host_to_device": (i32, [i32]),
    "lsa_ctx_destroy": (None, [vp]),
    "lsa_last_error": (s, [vp]),
    "lsa_sync": (i32, [vp]),
    "lsa_upload_frame": (i32, [vp, vp, i32]),
    "lsa_upload_wire_frame": (i32, [vp, vp, i32, vp, vp, i32, i32, f64, i32]),
    "lsa_upload_robosense_frame": (i32, [vp, vp, i32, i32, vp, vp, i32, i32, f64, vp]),
    "lsa_upload_polydata_frame": (i32, [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, vp, i32, f64, vp, vp]),
    "lsa_frame_store_put": (i32, [vp, i32, vp, i32]),
    "lsa_frame_store_use": (i32, [vp, i32]),
    "lsa_frame_size": (i32, [vp]),
    "lsa_get_azimuthal_resolution": (f32, [vp]),
    "lsa_set_azimuthal_resolution": (None, [vp, f32]),
    "lsa_extract_keypoints": (i32, [vp, P(ExtractParams), vp]),
    "lsa_extract_keypoints_more": (i32, [vp, P(ExtractParams), vp, f64, vp]),
    "lsa_upload_frame_begin": (i32, [vp, vp, i32]),
    "lsa_upload_frame_ready": (i32, [vp]),
    "lsa_upload_frame_adopt": (i32, [vp, vp, i32]),
    "lsa_pin_host_memory": (i32, [vp, sz]),
    "lsa_unpin_host_memory": (i32, [vp]),
    "lsa_upload_frame_forget": (i32, [vp]),
    "lsa_collect_garbage": (i32, [vp]),
    "lsa_uploads_adopted": (i32, [vp]),
    "lsa_extract_prefetch_uploaded": (i32, [vp, P(ExtractParams)]),
    "lsa_extract_prefetch": (i32, [vp, i32, P(ExtractParams)]),
    "lsa_extract_prefetch_adopted": (i32, [vp]),
    "lsa_set_keypoint_types": (i32, [vp, u32]),
    "lsa_download_keypoints": (i32, [vp, i32, i32, vp, i32]),
    "lsa_keypoint_count": (i32, [vp, i32, i32]),
    "lsa_download_debug": (i32, [vp, i32, vp, i32]),
    "lsa_nb_laser_rings": (i32, [vp]),
    "lsa_transform_keypoints": (i32, [vp, i32, i32, vp, f64]),
    # ---- targets and matching
    "lsa_set_target": (i32, [vp, i32, i32, vp, i32]),
    "lsa_target_staging": (vp, [vp, i32, i32, i32]),
    "lsa_set_target_staged": (i32, [vp, i32, i32, i32]),
    "lsa_stage_target_ahead": (i32, [vp, i32, i32, i32]),
    "lsa_drop_target_ahead": (i32, [vp, i32, i32]),
    "lsa_staged_targets_adopted": (i32, [vp]),
    "lsa_set_target_from_set": (i32, [vp, i32, i32, i32]),
    "lsa_prepare_previous_targets": (i32, [vp, u32]),
    "lsa_prepared_targets_adopted": (i32, [vp]),
    "lsa_target_size": (i32, [vp, i32, i32]),
    "lsa_download_target": (i32, [vp, i32, i32, vp, i32]),
    "lsa_set_target_cell_size": (i32, [vp, i32, i32, f32]),
    "lsa_set_knn_lanes": (i32, [vp, i32, i32]),
    "lsa_set_knn_rounds": (i32, [vp, i32, i32]),
    "lsa_match_serial": (i64, [vp, i32]),
    "lsa_match_histogram": (i32, [vp, i32, i64, vp]),
    "lsa_match_types_undistorted": (i32, [vp, i32, u32, P(MatchParams), vp, vp, vp, vp, f64, f64]),
    "lsa_set_fused_match": (i32, [vp, i32]),
    "lsa_match_slow_queries": (i32, [vp]),
    "lsa_match_route_stats": (i32, [vp, i32, vp]),
    "lsa_match_trace": (i32, [vp, vp, i32]),
    "lsa_match_exhaustive_queries": (i32, [vp]),
    "lsa_set_keypoints": (i32, [vp, i32, i32, vp, i32]),
    "lsa_match": (i32, [vp, i32, i32, i32, P(MatchParams), vp, vp]),
    "lsa_match_types": (i32, [vp, i32, u32, i32, P(MatchParams), vp, vp]),
    "lsa_overlap": (i32, [vp, u32, i32, vp, vp, f64, f64, f32, vp, vp]),
    "lsa_download_match": (i32, [vp, i32, vp, vp, vp, i32]),
    "lsa_upload_match": (i32, [vp, i32, vp, vp, i32, f64]),
    "lsa_download_knn": (i32, [vp, i32, vp, vp, vp, i32]),
    # ---- normal equations, solves, ICP links
    "lsa_accumulate": (i32, [vp, u32, vp, i32, vp, vp, vp, vp]),
    "lsa_mailbox_active": (i32, [vp]),
    "lsa_solve": (i32, [vp, u32, vp, i32, i32, vp, vp, vp]),
    "lsa_solve_device": (i32, [vp, u32, vp, i32, i32, i32, P(SolveResult)]),
    "lsa_solve_device_begin": (i32, [vp, u32, vp, i32, i32, i32]),
    "lsa_solve_device_end": (i32, [vp, vp]),
    "lsa_solve_device_drop": (i32, [vp]),
    "lsa_icp_cancel": (i32, [vp, i32]),
    "lsa_icp_abandon": (i32, [vp]),
    "lsa_match_types_linked": (i32, [vp, i32, u32, i32, vp, i32]),
    "lsa_icp_link": (i32, [vp]),
    "lsa_solve_device_begin_linked": (i32, [vp, u32, vp, i32, i32, i32, i32, vp]),
    "lsa_icp_link_peek": (i32, [vp, i32, vp]),
    "lsa_icp_link_expected": (i32, [vp, i32, i32, vp, vp, vp]),
    "lsa_solve_device_trace": (i32, [vp, vp]),
    "lsa_debug_set": (i32, [vp, s, i32]),
    "lsa_solve_device_shape": (i32, [vp, vp]),
    "lsa_accumulate_shape": (i32, [vp, vp]),
    "lsa_solve_device_fallbacks": (i32, [vp]),
    "lsa_solve_device_interlude": (i32, [vp, C.CFUNCTYPE(None, vp), vp]),
    "lsa_registration_error": (i32, [vp, u32, vp, i32, vp, vp]),
    # ---- external sensors
    "lsa_set_sensor_terms": (i32, [vp, vp]),
    "lsa_sensor_terms_eval": (i32, [vp, vp, vp]),
    "lsa_sensors_create": (vp, []),
    "lsa_sensors_destroy": (None, [vp]),
    "lsa_sensors_add_wheel_odom": (i32, [vp, f64, f64]),
    "lsa_sensors_add_gravity": (i32, [vp, f64, vp]),
    "lsa_sensors_set_weights": (i32, [vp, f64, f64]),
    "lsa_sensors_set_time_offset": (i32, [vp, f64]),
    "lsa_sensors_clear": (i32, [vp]),
    "lsa_sensors_compute": (i32, [vp, f64, vp]),
    "lsa_sensors_gravity_ref": (i32, [vp, vp]),
    # ---- undistortion, boxes, transforms
    "lsa_reset_working_keypoints": (i32, [vp]),
    "lsa_undistort": (i32, [vp, vp, vp, f64, f64]),
    "lsa_localization_begin": (i32, [vp, vp, vp, f64, f64, vp]),
    "lsa_arm_localization_boxes": (i32, [vp]),
    "lsa_working_time_range": (i32, [vp, vp, vp]),
    "lsa_keypoint_time_range": (i32, [vp, i32, vp, vp]),
    "lsa_working_bbox": (i32, [vp, i32, vp, vp, vp]),
    "lsa_working_bboxes": (i32, [vp, vp, vp, vp]),
    "lsa_keypoint_bboxes_begin": (i32, [vp, i32, vp]),
    "lsa_keypoint_bboxes_begin_interp": (i32, [vp, i32, vp, vp, f64, f64]),
    "lsa_keypoint_bboxes_end": (i32, [vp, vp, vp]),
    "lsa_keypoint_boxes_predicted_mark": (i32, [vp]),
    "lsa_keypoint_boxes_predicted": (i32, [vp, i32, vp, vp, f64, f64]),
    "lsa_download_transformed": (i32, [vp, i32, i32, vp, vp, i32]),
    "lsa_stage_transformed": (i32, [vp, i32, vp]),
    "lsa_staged_transformed": (i32, [vp, i32, vp, vp]),
    "lsa_transform_frame": (i32, [vp, i32, vp, vp, f64, f64, vp, i32]),
    "lsa_transform_frame_at": (i32, [vp, i32, vp, vp, f64, f64, f64, vp, i32]),
    # ---- self tests and profiling
    "lsa_selftest_math": (i32, [vp, i32, vp, vp, i32, vp]),
    "lsa_selftest_numerics": (i32, [vp, i32, vp, i32, vp]),
    "lsa_selftest_lm_step": (i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    "lsa_selftest_lm_host": (i32, [i32, vp, vp, vp, vp, vp, vp]),
    "lsa_selftest_labels": (i32, [vp, P(ExtractParams), vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "lsa_selftest_keep_busy": (i32, [vp, i32, i32]),
    "lsa_profile_enable": (i32, [vp, i32]),
    "lsa_profile_event_overhead_us": (f64, [vp]),
    "lsa_profile_select": (i32, [vp, s, i32]),
    "lsa_profile_reset": (i32, [vp]),
    "lsa_profile_get": (i32, [vp, vp, i32]),
    # ---- the pipeline
    "lsa_slam_create": (i32, [i32, P(vp)]),
    "lsa_slam_destroy": (None, [vp]),
    "lsa_slam_last_error": (s, [vp]),
    "lsa_slam_set_param": (i32, [vp, s, f64]),
    "lsa_slam_get_param": (i32, [vp, s, vp]),
    "lsa_slam_reset": (None, [vp, i32]),
    "lsa_slam_clear_maps": (i32, [vp]),
    "lsa_slam_add_frame": (i32, [vp, vp, i32, u64, u32]),
    "lsa_slam_store_frame": (i32, [vp, i32, vp, i32]),
    "lsa_slam_add_stored_frame": (i32, [vp, i32, u64, u32]),
    "lsa_slam_hint_next_stored_frame": (i32, [vp, i32]),
    "lsa_slam_hint_next_frame": (i32, [vp, vp, i32]),
    "lsa_slam_get_world_transform": (i32, [vp, vp, vp]),
    "lsa_slam_get_covariance": (i32, [vp, vp]),
    "lsa_slam_get_keypoints": (i32, [vp, i32, i32, vp, i32]),
    "lsa_slam_get_registered_frame": (i32, [vp, vp, i32]),
    "lsa_slam_get_match_status": (i32, [vp, i32, i32, vp, vp, i32]),
    "lsa_slam_get_stats": (i32, [vp, vp]),
    "lsa_slam_get_latency_compensated_world_transform": (i32, [vp, vp, vp]),
    "lsa_slam_add_frames": (i32, [vp, vp, vp, vp, vp, i32]),
    "lsa_slam_set_extractor_param": (i32, [vp, i32, s, f64]),
    "lsa_slam_get_extractor_param": (i32, [vp, i32, s, vp]),
    "lsa_slam_set_base_to_lidar_offset": (i32, [vp, vp, i32]),
    "lsa_slam_get_base_to_lidar_offset": (i32, [vp, vp, i32]),
    "lsa_slam_set_world_transform_from_guess": (i32, [vp, vp]),
    "lsa_slam_get_trajectory": (i32, [vp, vp, vp, i32]),
    "lsa_slam_get_debug_information": (i32, [vp, vp]),
    "lsa_slam_get_map": (i32, [vp, i32, i32, vp, i32]),
    "lsa_slam_get_target_submap": (i32, [vp, i32, vp, i32]),
    "lsa_slam_context": (vp, [vp]),
    "lsa_slam_add_wheel_odom_measurement": (i32, [vp, f64, f64]),
    "lsa_slam_add_gravity_measurement": (i32, [vp, f64, vp]),
    "lsa_slam_clear_sensor_measurements": (i32, [vp]),
    "lsa_slam_sensor_terms": (i32, [vp, vp]),
    "lsa_slam_add_map_points": (i32, [vp, i32, vp, i32, i32, f64]),
    "lsa_slam_save_maps_pcd": (i32, [vp, s, i32, i32]),
    "lsa_slam_load_maps_pcd": (i32, [vp, s, i32, f64]),
    "lsa_slam_map_io_counts": (i32, [vp, vp]),
    "lsa_slam_set_trajectory_and_rebuild_maps": (i32, [vp, vp, i32]),
    "lsa_slam_logged_frames": (i32, [vp]),
    "lsa_slam_get_logged_keypoints": (i32, [vp, i32, i32, vp, i32]),
    # ---- loop closure and place recognition
    "lsa_loop_closure_params_init": (None, [vp]),
    "lsa_slam_register_logged_frames": (i32, [vp, i32, i32, vp, vp, vp]),
    "lsa_loop_closure_candidate": (i32, [vp, i32, i32, f64, f64]),
    "lsa_place_params_init": (None, [vp]),
    "lsa_place_search_init": (None, [vp]),
    "lsa_scan_descriptor_host": (i32, [vp, vp, i32, vp]),
    "lsa_place_distance_host": (i32, [vp, vp, vp, vp, vp]),
    "lsa_place_select_host": (i32, [vp, vp, vp, i32, i32, i32, f64, f64, f64, i32, vp, i32]),
    "lsa_slam_recognize_place": (i32, [vp, i32, vp, vp, i32]),
    "lsa_loop_detect_init": (None, [vp]),
    "lsa_place_detect_host": (i32, [vp, vp, vp, i32, vp, i32]),
    "lsa_slam_detect_loop_closures": (i32, [vp, vp, vp, i32]),
    "lsa_map_place_search_init": (None, [vp]),
    "lsa_map_descriptor_host": (i32, [vp, vp, i32, vp, vp]),
    "lsa_map_place_select_host": (i32, [vp, vp, vp, i32, i32, vp, vp, i32]),
    "lsa_slam_recognize_place_in_maps": (i32, [vp, vp, i32, vp, vp, i32, vp]),
    # ---- device maps
    "lsa_device_grid_create": (i32, [vp, P(vp)]),
    "lsa_device_grid_destroy": (None, [vp]),
    "lsa_device_grid_set": (i32, [vp, s, f64]),
    "lsa_device_grid_get_param": (f64, [vp, s]),
    "lsa_device_grid_reset": (i32, [vp, vp]),
    "lsa_device_grid_clear": (i32, [vp]),
    "lsa_device_grid_size": (i32, [vp]),
    "lsa_device_grid_add": (i32, [vp, vp, i32, i32, f64, i32]),
    "lsa_device_grid_add_keypoints": (i32, [vp, i32, i32, vp, f64]),
    "lsa_device_grid_stage_keypoints": (i32, [vp, i32, i32, vp]),
    "lsa_device_grid_add_staged": (i32, [vp, f64]),
    "lsa_device_grid_stage_keypoints_all": (i32, [vp, vp, i32, i32, vp]),
    "lsa_device_grid_add_staged_all": (i32, [vp, i32, f64]),
    "lsa_device_grid_roll": (i32, [vp, vp, vp]),
    "lsa_device_grid_clear_old_points": (i32, [vp, f64]),
    "lsa_device_grid_get": (i32, [vp, i32, vp, i32]),
    "lsa_device_grid_build_submap": (i32, [vp, vp, vp, i32, i32, i32]),
    "lsa_device_grid_build_submap_begin": (i32, [vp, vp, vp, i32, i32, i32]),
    "lsa_device_grid_build_submap_begin_for_keypoints": (i32, [vp, i32, i32, i32, i32]),
    "lsa_device_grid_build_submap_end": (i32, [vp]),
    "lsa_device_grid_submap_valid": (i32, [vp]),
    "lsa_device_grid_submap_ahead_begin": (i32, [vp, i32, i32, i32]),
    "lsa_device_grid_submap_ahead_poll": (i32, [vp]),
    "lsa_device_grid_submap_ahead_poll_all": (i32, [vp, i32]),
    "lsa_device_grid_submap_ahead_wait": (i32, [vp]),
    "lsa_device_grid_submap_ahead_take": (i32, [vp, i32, i32, i32, i32, vp]),
    "lsa_device_grid_submap_ahead_take_begin": (i32, [vp, i32, i32, i32, i32]),
    "lsa_device_grid_submap_ahead_take_end": (i32, [vp, vp]),
    "lsa_device_grid_add_pcd": (i32, [vp, s, i32, f64, i32]),
    "lsa_device_grid_save_pcd": (i32, [vp, s, i32, i32]),
    "lsa_pcd_io_times": (i32, [vp, vp]),
    # ---- the dense point-cloud map
    "lsa_dense_map_create": (i32, [vp, f64, P(vp)]),
    "lsa_dense_map_destroy": (None, [vp]),
    "lsa_dense_map_set": (i32, [vp, s, f64]),
    "lsa_dense_map_get_param": (f64, [vp, s]),
    "lsa_dense_map_insert_points": (i32, [vp, vp, i32, i32]),
    "lsa_dense_map_insert_frame": (i32, [vp, i32, vp, vp, f64, f64, f64, i32]),
    "lsa_dense_map_reserve": (i32, [vp, i64]),
    "lsa_dense_map_size": (i32, [vp]),
    "lsa_dense_map_skipped": (i64, [vp]),
    "lsa_dense_map_bytes": (i64, [vp]),
    "lsa_dense_map_get": (i32, [vp, i32, vp, vp, i32]),
    "lsa_dense_map_get_sources": (i32, [vp, i32, vp, i32]),
    "lsa_dense_map_reproject": (i32, [vp, vp, i32, i32, P(i64)]),
    "lsa_pose_corrections": (i32, [vp, vp, i32, vp]),
    "lsa_slam_get_dense_map_sources": (i32, [vp, i32, vp, i32]),
    "lsa_dense_map_clear": (i32, [vp]),
    "lsa_dense_map_save_pcd": (i32, [vp, s, i32, i32]),
    "lsa_slam_dense_map_size": (i32, [vp]),
    "lsa_slam_get_dense_map": (i32, [vp, i32, vp, vp, i32]),
    "lsa_slam_save_dense_map_pcd": (i32, [vp, s, i32, i32]),
    "lsa_slam_clear_dense_map": (i32, [vp]),
    "lsa_dense_map_carve_points": (i32, [vp, vp, i32, vp, i32, i32]),
    "lsa_dense_map_carve_frame": (i32, [vp, i32, vp, vp, f64, f64, f64, i32]),
    "lsa_transform_frame_origins_at": (i32, [vp, i32, vp, vp, f64, f64, f64, vp, i32]),
    "lsa_dense_map_get_filtered": (i32, [vp, i32, f64, vp, vp, i32]),
    "lsa_dense_map_get_sources_filtered": (i32, [vp, i32, f64, vp, i32]),
    "lsa_dense_map_get_misses": (i32, [vp, i32, f64, vp, i32]),
    "lsa_dense_map_prune": (i32, [vp, i32, f64, P(i64)]),
    "lsa_dense_map_save_pcd_filtered": (i32, [vp, s, i32, i32, f64]),
    "lsa_slam_get_dense_map_filtered": (i32, [vp, i32, f64, vp, vp, i32]),
    "lsa_slam_get_dense_map_misses": (i32, [vp, i32, f64, vp, i32]),
    "lsa_slam_save_dense_map_pcd_filtered": (i32, [vp, s, i32, i32, f64]),
    "lsa_slam_prune_dense_map": (i32, [vp, i32, f64, P(i64)]),
    "lsa_dense_map_get_normals": (i32, [vp, i32, f64, i32, i32, vp, i32, i32, vp, i32]),
    "lsa_dense_map_save_pcd_normals": (i32, [vp, s, i32, i32, f64, i32, i32, vp, i32, i32]),
    "lsa_pcd_read_normals": (i32, [s, vp, i32]),
    "lsa_slam_get_dense_map_normals": (i32, [vp, i32, f64, i32, i32, i32, vp, i32]),
    "lsa_slam_save_dense_map_pcd_normals": (i32, [vp, s, i32, i32, f64, i32, i32, i32]),
    "lsa_slam_get_dense_map_viewpoints": (i32, [vp, vp, i32, P(i32)]),
    "lsa_slam_get_registered_frame_origins": (i32, [vp, vp, i32]),
    # ---- the keypoint log and its descriptor store
    "lsa_kplog_describe": (i32, [vp, vp, i32, i32]),
    "lsa_kplog_descriptors": (i32, [vp, i32, i32, vp]),
    "lsa_kplog_place_search": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "lsa_kplog_described": (i32, [vp]),
    "lsa_kplog_descriptor_length": (i32, [vp]),
    "lsa_kplog_place_search_rows": (i32, [vp, vp, i32, i32, i32, vp, vp]),
    "lsa_kplog_detect_loops": (i32, [vp, vp, vp, i32, vp, i32]),
    "lsa_kplog_append": (i32, [vp]),
    "lsa_kplog_append_points": (i32, [vp, vp, vp]),
    "lsa_kplog_pop_front": (i32, [vp]),
    "lsa_kplog_clear": (i32, [vp]),
    "lsa_kplog_size": (i32, [vp]),
    "lsa_kplog_count": (i32, [vp, i32, i32]),
    "lsa_kplog_get": (i32, [vp, i32, i32, vp, i32]),
    "lsa_kplog_bytes": (ull, [vp]),
    "lsa_kplog_stopped": (i32, [vp]),
    "lsa_kplog_replay": (i32, [vp, u32, vp, vp, i32, i32, vp, vp, vp]),
    "lsa_kplog_replayed": (i64, [vp, i32, vp]),
    "lsa_kplog_replay_to_grids": (i32, [vp, u32, vp, vp, i32, i32, vp, vp, vp]),
    "lsa_kplog_replay_range": (i32, [vp, u32, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
    # ---- the table of map descriptors
    "lsa_map_place_describe_points": (i32, [vp, vp, vp, i32, vp, i32]),
    "lsa_map_place_describe_grids": (i32, [vp, vp, vp, vp, i32]),
    "lsa_map_place_descriptors": (i32, [vp, i32, i32, vp]),
    "lsa_map_place_search": (i32, [vp, vp, i32, vp, vp]),
    "lsa_map_place_slices": (i32, [vp, vp, i32]),
    "lsa_map_place_viewpoints": (i32, [vp]),
    # ---- pose graph
    "lsa_pgo_params_init": (None, [vp]),
    "lsa_pgo_solve_host": (i32, [vp, i32, vp, vp, i32, vp, vp, vp]),
    "lsa_pgo_solve": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, vp]),
    "lsa_pgo_linearize_host": (i32, [vp, i32, vp, i32, vp, vp, vp]),
    "lsa_pgo_linearize": (i32, [vp, vp, i32, vp, i32, vp, vp, vp]),
    "lsa_pgo_assemble_host": (i32, [vp, i32, vp, vp, i32, f64, vp, vp, vp, vp]),
    "lsa_pgo_assemble": (i32, [vp, vp, i32, vp, vp, i32, f64, vp, vp, vp, vp]),
    "lsa_pgo_tridiagonal_solve_host": (i32, [i32, vp, vp, vp, vp, vp]),
    "lsa_pgo_tridiagonal_solve": (i32, [vp, i32, vp, vp, vp, vp, vp]),
    "lsa_pgo_spmv_host": (i32, [vp, i32, vp, vp, i32, f64, vp, vp]),
    "lsa_pgo_spmv": (i32, [vp, vp, i32, vp, vp, i32, f64, vp, vp]),
    "lsa_pgo_retract_host": (i32, [vp, i32, vp, vp]),
    "lsa_pgo_retract": (i32, [vp, vp, i32, vp, vp]),
    "lsa_pgo_edge_jacobians_host": (i32, [vp, i32, vp, vp, vp, vp]),
    "lsa_pgo_information_from_covariance": (i32, [vp, vp]),
    "lsa_slam_optimize_logged_trajectory": (i32, [vp, vp, i32, vp, vp, i32, vp]),
    "lsa_pgo_solve_priors_host": (i32, [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]),
    "lsa_pgo_solve_priors": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]),
    "lsa_pgo_linearize_priors_host": (i32, [vp, i32, vp, i32, vp, vp, vp, vp]),
    "lsa_pgo_linearize_priors": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, vp]),
    "lsa_pgo_assemble_priors_host": (i32, [vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp, vp, vp]),
    "lsa_pgo_assemble_priors": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp, vp, vp]),
    "lsa_pgo_spmv_priors_host": (i32, [vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp]),
    "lsa_pgo_spmv_priors": (i32, [vp, vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp]),
    "lsa_pgo_prior_jacobian_host": (i32, [vp, i32, vp, vp, vp, vp]),
    "lsa_pgo_premultiply_host": (i32, [vp, i32, vp, vp]),
    "lsa_pgo_premultiply": (i32, [vp, vp, i32, vp, vp]),
    "lsa_pgo_reanchor_host": (i32, [vp, i32, vp]),
    "lsa_pgo_reanchor": (i32, [vp, vp, i32, vp]),
    "lsa_pgo_information_from_covariance3": (i32, [vp, vp]),
    "lsa_gps_match_trajectory": (i32, [vp, i32, vp, i32, f64, f64, vp]),
    "lsa_trajectory_alignment": (i32, [vp, vp, i32, vp]),
    "lsa_slam_run_pose_graph_optimization": (i32, [vp, vp, vp, vp, i32, vp, f64, vp, vp, i32, vp]),
    "lsa_pgo_robust_init": (None, [vp]),
    "lsa_pgo_robust_rho_host": (i32, [i32, f64, f64, vp, vp]),
    "lsa_pgo_linearize_robust_host": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "lsa_pgo_linearize_robust": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "lsa_pgo_linearize_robust_priors_host": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "lsa_pgo_linearize_robust_priors": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "lsa_pgo_solve_robust_host": (i32, [vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "lsa_pgo_solve_robust": (i32, [vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "lsa_slam_optimize_logged_trajectory_robust": (i32, [vp, vp, i32, vp, vp, vp, i32, vp, vp]),
    "lsa_slam_run_pose_graph_optimization_robust": (i32, [vp, vp, vp, vp, i32, vp, f64, vp, vp, vp, i32, vp, vp]),
    "lsa_slam_close_loops": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32]),
    # ---- host maps
    "lsa_rolling_grid_create": (vp, []),
    "lsa_rolling_grid_destroy": (None, [vp]),
    "lsa_rolling_grid_set": (i32, [vp, s, f64]),
    "lsa_rolling_grid_reset": (None, [vp, vp]),
    "lsa_rolling_grid_clear": (None, [vp]),
    "lsa_rolling_grid_size": (i32, [vp]),
    "lsa_rolling_grid_roll": (None, [vp, vp, vp]),
    "lsa_rolling_grid_add": (i32, [vp, vp, i32, i32, f64, i32]),
    "lsa_rolling_grid_clear_old_points": (None, [vp, f64]),
    "lsa_rolling_grid_get": (i32, [vp, i32, vp, i32]),
    "lsa_rolling_grid_build_submap": (i32, [vp, vp, vp, i32]),
    "lsa_rolling_grid_submap_valid": (i32, [vp]),
    "lsa_rolling_grid_submap": (i32, [vp, vp, i32]),
    # ---- PCD files
    "lsa_pcd_info": (i32, [s, P(i32), P(i32)]),
    "lsa_pcd_read": (i32, [s, vp, i32]),
    "lsa_pcd_write": (i32, [s, vp, i32, i32]),
    "lsa_pcd_last_error": (s, []),
    "lsa_lzf_compress": (i32, [vp, sz, vp, sz, P(sz)]),
    "lsa_lzf_decompress": (i32, [vp, sz, vp, sz, P(sz)]),
    # ---- the synthetic generator (libslamsynth.so exports the same three: _native.synth_lib)
    "lsa_synth_sensor": (i32, [i32, P(i32), P(i32), P(f64), P(f64)]),
    "lsa_synth_frame": (i32, [i32, u64, i32, vp, i32, P(u64)]),
    "lsa_synth_pose": (None, [i32, vp]),
}

# every symbol include/lidarslam_amd.h declares (tests/test_abi.py checks the .so exports them all)
ABI_SYMBOLS = list(SIGNATURES)


def declare(L, names=SIGNATURES):
    """Gives the functions `names` of the loaded library L their signatures from the table."""
    for name in names:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = SIGNATURES[name]
    return L


_lib = None


def lib():
    """Loads liblidarslam_amd.so (built in-tree by __graft_entry__.build()); raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LsaError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    _lib = declare(C.CDLL(LIB_PATH))
    return _lib
