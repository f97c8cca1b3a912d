"""lidarslam_amd -- MI355X-native scan-matching hot path of Perception4D/LidarSlam.

Python front-end (ctypes) of liblidarslam_amd.so.  Two levels, both thin:

* :class:`Context`  -- the kernel-level C ABI (include/lidarslam_amd.h): upload a scan, extract
  keypoints, set a kNN target, match, accumulate normal equations, undistort.
* :class:`Slam`     -- the pipeline: ``add_frame`` / ``world_transform`` mirror
  ``LidarSlam::Slam::AddFrame`` / ``GetWorldTransform`` (slam_lib/include/LidarSlam/Slam.h:111-146).

There is no CPU fallback: without the built library or without a HIP device every constructor
raises.  The CPU oracle under ``oracle/`` is test infrastructure and is never imported from here.
"""
import ctypes as C
import os

import numpy as np

from ._native import (  # noqa: F401
    BLOB,
    EDGE,
    LIB_PATH,
    MATCH_NSTATUS,
    PLANE,
    POINT_DTYPE,
    SET_RAW_CURRENT,
    SET_RAW_PREVIOUS,
    SET_WORKING,
    ExtractParams,
    KernelStat,
    MatchParams,
    pose16,
    ptr,
    synth_frame,
    synth_pose,
)

__all__ = ["Context", "Slam", "ExtractParams", "MatchParams", "POINT_DTYPE", "lib", "LsaError", "read_pcd", "write_pcd"]

TARGET_MAP, TARGET_PREVIOUS = 0, 1
KNN_MAX = 16  # LSA_KNN_MAX: slots per query of the neighbour lists (Context.knn_lists)

DEBUG_INFORMATION_NAMES = [
    "EgoMotion: edges used", "EgoMotion: planes used", "Localization: edges used", "Localization: planes used",
    "Localization: blobs used", "Localization: position error", "Localization: orientation error",
    "Confidence: overlap", "Confidence: comply motion limits", "latency",
]

DEBUG_NAMES = [
    "sin_angle", "saliency", "depth_gap", "intensity_gap", "edge_keypoint", "plane_keypoint", "blob_keypoint",
    "edge_validity", "plane_validity", "blob_validity",
]

# every symbol include/lidarslam_amd.h declares (tests/test_abi.py checks the .so exports them all)
ABI_SYMBOLS = [
    "lsa_device_count", "lsa_bind_host_to_device", "lsa_ctx_create", "lsa_ctx_destroy", "lsa_last_error", "lsa_sync", "lsa_upload_frame", "lsa_upload_wire_frame", "lsa_upload_polydata_frame",
    "lsa_frame_store_put", "lsa_frame_store_use", "lsa_frame_size", "lsa_get_azimuthal_resolution",
    "lsa_set_azimuthal_resolution", "lsa_extract_keypoints", "lsa_extract_keypoints_more", "lsa_extract_prefetch", "lsa_extract_prefetch_adopted", "lsa_transform_frame_at", "lsa_set_keypoint_types", "lsa_download_keypoints", "lsa_keypoint_count",
    "lsa_download_debug", "lsa_nb_laser_rings", "lsa_transform_keypoints", "lsa_set_target", "lsa_set_target_from_set", "lsa_prepare_previous_targets", "lsa_prepared_targets_adopted", "lsa_target_staging", "lsa_set_target_staged", "lsa_stage_target_ahead", "lsa_drop_target_ahead", "lsa_staged_targets_adopted",
    "lsa_target_size", "lsa_download_target", "lsa_set_target_cell_size", "lsa_set_knn_lanes", "lsa_set_fused_match", "lsa_set_knn_rounds", "lsa_match_slow_queries", "lsa_match_exhaustive_queries", "lsa_match_route_stats", "lsa_match_trace", "lsa_set_keypoints", "lsa_match", "lsa_match_types", "lsa_match_types_undistorted",
    "lsa_download_match", "lsa_upload_match", "lsa_download_knn", "lsa_overlap", "lsa_accumulate", "lsa_mailbox_active", "lsa_solve", "lsa_solve_device", "lsa_solve_device_fallbacks", "lsa_solve_device_begin", "lsa_solve_device_end", "lsa_solve_device_drop", "lsa_icp_link", "lsa_solve_device_begin_linked", "lsa_icp_link_peek", "lsa_icp_link_expected", "lsa_icp_cancel", "lsa_icp_abandon", "lsa_debug_set", "lsa_solve_device_shape", "lsa_accumulate_shape", "lsa_match_types_linked", "lsa_solve_device_trace", "lsa_registration_error", "lsa_selftest_math", "lsa_selftest_numerics", "lsa_selftest_labels", "lsa_reset_working_keypoints", "lsa_undistort", "lsa_working_time_range",
    "lsa_working_bbox", "lsa_working_bboxes", "lsa_localization_begin", "lsa_arm_localization_boxes", "lsa_keypoint_bboxes_begin", "lsa_keypoint_bboxes_begin_interp", "lsa_keypoint_boxes_predicted_mark", "lsa_keypoint_boxes_predicted", "lsa_keypoint_time_range", "lsa_keypoint_bboxes_end", "lsa_download_transformed", "lsa_stage_transformed", "lsa_staged_transformed", "lsa_transform_frame", "lsa_profile_enable", "lsa_profile_select", "lsa_profile_reset",
    "lsa_profile_get", "lsa_slam_create", "lsa_slam_destroy", "lsa_slam_last_error", "lsa_slam_set_param",
    "lsa_slam_get_param", "lsa_slam_reset", "lsa_slam_clear_maps", "lsa_slam_add_frame", "lsa_slam_store_frame", "lsa_slam_add_stored_frame", "lsa_slam_hint_next_stored_frame", "lsa_slam_hint_next_frame", "lsa_upload_frame_begin", "lsa_upload_frame_ready", "lsa_upload_frame_adopt", "lsa_upload_frame_forget", "lsa_profile_event_overhead_us", "lsa_upload_robosense_frame", "lsa_pin_host_memory", "lsa_unpin_host_memory", "lsa_collect_garbage", "lsa_uploads_adopted", "lsa_extract_prefetch_uploaded",
    "lsa_slam_get_world_transform", "lsa_slam_get_covariance", "lsa_slam_get_keypoints", "lsa_slam_get_registered_frame",
    "lsa_slam_get_match_status", "lsa_slam_get_stats", "lsa_slam_context", "lsa_slam_get_latency_compensated_world_transform",
    "lsa_slam_set_world_transform_from_guess", "lsa_slam_get_trajectory", "lsa_slam_get_debug_information", "lsa_slam_get_map",
    "lsa_slam_get_target_submap", "lsa_slam_set_base_to_lidar_offset", "lsa_slam_get_base_to_lidar_offset", "lsa_slam_add_frames", "lsa_slam_set_extractor_param", "lsa_slam_get_extractor_param", "lsa_match_serial", "lsa_match_histogram", "lsa_synth_sensor", "lsa_synth_frame",
    "lsa_synth_pose",
    "lsa_selftest_keep_busy", "lsa_solve_device_interlude", "lsa_device_grid_create", "lsa_device_grid_destroy", "lsa_device_grid_set", "lsa_device_grid_get_param", "lsa_device_grid_reset", "lsa_device_grid_clear",
    "lsa_device_grid_size", "lsa_device_grid_add", "lsa_device_grid_add_keypoints", "lsa_device_grid_roll", "lsa_device_grid_clear_old_points",
    "lsa_device_grid_get", "lsa_device_grid_build_submap", "lsa_device_grid_submap_valid", "lsa_device_grid_stage_keypoints", "lsa_device_grid_stage_keypoints_all", "lsa_device_grid_add_staged", "lsa_device_grid_add_staged_all",
    "lsa_device_grid_build_submap_begin", "lsa_device_grid_build_submap_begin_for_keypoints", "lsa_device_grid_build_submap_end",
    "lsa_device_grid_submap_ahead_begin", "lsa_device_grid_submap_ahead_poll", "lsa_device_grid_submap_ahead_poll_all", "lsa_device_grid_submap_ahead_wait", "lsa_device_grid_submap_ahead_take", "lsa_device_grid_submap_ahead_take_begin", "lsa_device_grid_submap_ahead_take_end",
    "lsa_rolling_grid_create", "lsa_rolling_grid_destroy", "lsa_rolling_grid_set", "lsa_rolling_grid_reset", "lsa_rolling_grid_clear",
    "lsa_rolling_grid_size", "lsa_rolling_grid_roll", "lsa_rolling_grid_add", "lsa_rolling_grid_clear_old_points", "lsa_rolling_grid_get",
    "lsa_rolling_grid_build_submap", "lsa_rolling_grid_submap_valid", "lsa_rolling_grid_submap",
    "lsa_set_sensor_terms", "lsa_sensor_terms_eval", "lsa_sensors_create", "lsa_sensors_destroy", "lsa_sensors_add_wheel_odom",
    "lsa_sensors_add_gravity", "lsa_sensors_set_weights", "lsa_sensors_set_time_offset", "lsa_sensors_clear", "lsa_sensors_compute",
    "lsa_sensors_gravity_ref", "lsa_slam_add_wheel_odom_measurement", "lsa_slam_add_gravity_measurement",
    "lsa_slam_clear_sensor_measurements", "lsa_slam_sensor_terms",
    "lsa_pcd_info", "lsa_pcd_read", "lsa_pcd_write", "lsa_pcd_last_error", "lsa_lzf_compress", "lsa_lzf_decompress",
    "lsa_device_grid_add_pcd", "lsa_device_grid_save_pcd", "lsa_pcd_io_times",
    "lsa_slam_add_map_points", "lsa_slam_save_maps_pcd", "lsa_slam_load_maps_pcd", "lsa_slam_map_io_counts",
    "lsa_kplog_append", "lsa_kplog_append_points", "lsa_kplog_pop_front", "lsa_kplog_clear", "lsa_kplog_size", "lsa_kplog_count", "lsa_kplog_get",
    "lsa_kplog_bytes", "lsa_kplog_stopped", "lsa_kplog_replay", "lsa_kplog_replayed", "lsa_kplog_replay_to_grids",
    "lsa_slam_set_trajectory_and_rebuild_maps", "lsa_slam_logged_frames", "lsa_slam_get_logged_keypoints",
    "lsa_kplog_replay_range", "lsa_loop_closure_params_init", "lsa_slam_register_logged_frames", "lsa_loop_closure_candidate",
    "lsa_place_params_init", "lsa_place_search_init", "lsa_scan_descriptor_host", "lsa_place_distance_host", "lsa_place_select_host",
    "lsa_slam_recognize_place", "lsa_kplog_describe", "lsa_kplog_descriptors", "lsa_kplog_place_search", "lsa_kplog_described", "lsa_kplog_descriptor_length",
    "lsa_pgo_params_init", "lsa_pgo_solve_host", "lsa_pgo_solve", "lsa_pgo_linearize_host", "lsa_pgo_linearize", "lsa_pgo_assemble_host", "lsa_pgo_assemble",
    "lsa_pgo_tridiagonal_solve_host", "lsa_pgo_tridiagonal_solve", "lsa_pgo_spmv_host", "lsa_pgo_spmv", "lsa_pgo_information_from_covariance",
    "lsa_pgo_retract_host", "lsa_pgo_retract", "lsa_pgo_edge_jacobians_host", "lsa_slam_optimize_logged_trajectory",
    "lsa_pgo_solve_priors_host", "lsa_pgo_solve_priors", "lsa_pgo_linearize_priors_host", "lsa_pgo_linearize_priors", "lsa_pgo_assemble_priors_host",
    "lsa_pgo_assemble_priors", "lsa_pgo_spmv_priors_host", "lsa_pgo_spmv_priors", "lsa_pgo_prior_jacobian_host", "lsa_pgo_premultiply_host", "lsa_pgo_premultiply",
    "lsa_pgo_reanchor_host", "lsa_pgo_reanchor", "lsa_pgo_information_from_covariance3", "lsa_gps_match_trajectory", "lsa_trajectory_alignment",
    "lsa_slam_run_pose_graph_optimization",
]

PCD_ASCII, PCD_BINARY, PCD_BINARY_COMPRESSED = 0, 1, 2  # PCDFormat (PointCloudStorage.h:60-65)
PCD_FORMAT_NAMES = ["ascii", "binary", "binary_compressed"]


class LsaError(RuntimeError):
    code = None  # the LSA_E_* value of the call that failed, where there was one


E_NO_DEVICE, E_HIP, E_ARG, E_STATE, E_CAPACITY = -1, -2, -3, -4, -5


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


class LoopClosureParams(C.Structure):
    """lsa_loop_closure_params_t (include/lidarslam_amd.h): a value <= 0 of the last four means the Localization parameter
    of the same meaning."""

    _fields_ = [
        ("revisited_half_window", C.c_int32), ("query_half_window", C.c_int32), ("icp_max_iter", C.c_int32), ("lm_max_iter", C.c_int32),
        ("init_saturation", C.c_double), ("final_saturation", C.c_double),
    ]

    def __init__(self, revisited_half_window=5, query_half_window=0, icp_max_iter=0, lm_max_iter=0, init_saturation=0.0, final_saturation=0.0):
        super().__init__(revisited_half_window, query_half_window, icp_max_iter, lm_max_iter, init_saturation, final_saturation)


class LoopClosureResultStruct(C.Structure):
    """lsa_loop_closure_result_t (include/lidarslam_amd.h)."""

    _fields_ = [
        ("world", C.c_double * 16), ("relative", C.c_double * 16), ("covariance", C.c_double * 36),
        ("position_error", C.c_double), ("orientation_error", C.c_double), ("status", C.c_int32), ("iterations", C.c_int32),
        ("first_histogram", C.c_int32 * 24), ("last_histogram", C.c_int32 * 24), ("target_points", C.c_int64 * 3), ("query_points", C.c_int64 * 3),
    ]


class LoopClosureResult:
    """What Slam.register_logged_frames returns: world (4, 4), relative (4, 4) = inv(P[revisited]) @ world, covariance (6, 6),
    position_error [m], orientation_error [deg], status (0 registered, 1 skipped), iterations, first_histogram /
    last_histogram (3, 8) and target_points / query_points (3,)."""

    def __init__(self, r):
        self.world = np.array(r.world).reshape(4, 4)
        self.relative = np.array(r.relative).reshape(4, 4)
        self.covariance = np.array(r.covariance).reshape(6, 6)
        self.position_error, self.orientation_error = r.position_error, r.orientation_error
        self.status, self.iterations = r.status, r.iterations
        self.first_histogram = np.array(r.first_histogram, np.int32).reshape(3, 8)
        self.last_histogram = np.array(r.last_histogram, np.int32).reshape(3, 8)
        self.target_points = np.array(r.target_points, np.int64)
        self.query_points = np.array(r.query_points, np.int64)


def loop_closure_candidate(poses, times, query, min_travelled, max_distance):
    """lsa_loop_closure_candidate on a trajectory as Slam.trajectory() gives it (poses (n, 4, 4), times (n,)): among the
    frames before `query` at least min_travelled metres back along the trajectory and within max_distance metres of
    query's position, the nearest (the lower index on a tie); -1 when there is none.  Host only."""
    P = np.asarray(poses, np.float64).reshape(-1, 16)
    rows = np.ascontiguousarray(np.concatenate([P, np.asarray(times, np.float64).reshape(-1, 1)], axis=1))
    rc = lib().lsa_loop_closure_candidate(ptr(rows), rows.shape[0], int(query), float(min_travelled), float(max_distance))
    if rc < -1:
        raise _error("lsa_loop_closure_candidate", rc, "bad argument")
    return rc


class PlaceParams(C.Structure):
    """lsa_place_params_t (include/lidarslam_amd.h): the shape of a frame's descriptor.  min_common_sectors None: the default
    of the shape, max(1, sectors // 4)."""

    _fields_ = [
        ("rings", C.c_int32), ("sectors", C.c_int32), ("type_mask", C.c_uint32), ("min_common_sectors", C.c_int32),
        ("min_range", C.c_double), ("max_range", C.c_double), ("height_offset", C.c_double),
    ]

    def __init__(self, rings=20, sectors=60, type_mask=(1 << EDGE) | (1 << PLANE), min_range=0.0, max_range=80.0, height_offset=2.0, min_common_sectors=None):
        if min_common_sectors is None:
            min_common_sectors = max(1, int(sectors) // 4)
        super().__init__(rings, sectors, type_mask, min_common_sectors, min_range, max_range, height_offset)

    @property
    def length(self):
        """floats of a descriptor: rings * sectors cells, row-major [ring][sector], then the sectors column norms"""
        return self.rings * self.sectors + self.sectors


class PlaceSearch(C.Structure):
    """lsa_place_search_t: the descriptor's parameters and the selection's."""

    _fields_ = [
        ("descriptor", PlaceParams), ("min_travelled", C.c_double), ("max_distance", C.c_double), ("max_descriptor_distance", C.c_double),
        ("exclusion_half_window", C.c_int32), ("reserved", C.c_int32),
    ]

    def __init__(self, min_travelled=20.0, max_distance=0.0, max_descriptor_distance=0.0, exclusion_half_window=5, **descriptor):
        super().__init__(PlaceParams(**descriptor), min_travelled, max_distance, max_descriptor_distance, exclusion_half_window, 0)


class PlaceCandidateStruct(C.Structure):
    """lsa_place_candidate_t."""

    _fields_ = [("frame", C.c_int32), ("shift", C.c_int32), ("distance", C.c_float), ("reserved", C.c_float), ("yaw", C.c_double)]


def _candidates(out, n):
    """[(frame, distance, shift, yaw)]: distance a numpy float32, yaw a float [rad]"""
    return [(int(c.frame), np.float32(c.distance), int(c.shift), float(c.yaw)) for c in out[:n]]


def scan_descriptor(points, **params):
    """The host statement of a frame's descriptor (lsa_scan_descriptor_host): points a POINT_DTYPE array, or (n, 3) xyz,
    already filtered by type -> float32 (rings * sectors + sectors,).  params: PlaceParams' fields."""
    p = PlaceParams(**params)
    pts = np.asarray(points)
    if pts.dtype != POINT_DTYPE:
        xyz = np.asarray(points, np.float32).reshape(-1, 3)
        pts = np.zeros(xyz.shape[0], POINT_DTYPE)
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts = np.ascontiguousarray(pts)
    out = np.zeros(max(p.rings, 0) * max(p.sectors, 0) + max(p.sectors, 0), np.float32)
    rc = lib().lsa_scan_descriptor_host(C.byref(p), ptr(pts) if pts.size else None, pts.size, ptr(out))
    if rc < 0:
        raise _error("lsa_scan_descriptor_host", rc, "parameters out of limits")
    return out


def place_distance(a, b, **params):
    """The host statement of the distance of query descriptor a to candidate descriptor b (lsa_place_distance_host) ->
    (distance float32, shift): the smallest distance over the column shifts, the lowest shift on a tie."""
    p = PlaceParams(**params)
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1))
    b = np.ascontiguousarray(np.asarray(b, np.float32).reshape(-1))
    if p.rings < 1 or p.sectors < 1 or a.size != p.length or b.size != p.length:
        raise _error("lsa_place_distance_host", E_ARG, "descriptors of another shape than the parameters'")
    d, s = C.c_float(), C.c_int()
    rc = lib().lsa_place_distance_host(C.byref(p), ptr(a), ptr(b), C.byref(d), C.byref(s))
    if rc < 0:
        raise _error("lsa_place_distance_host", rc, "parameters out of limits")
    return np.float32(d.value), int(s.value)


def place_select(distance, shift, poses, times, query, sectors=60, min_travelled=20.0, max_distance=0.0, max_descriptor_distance=0.0,
                 exclusion_half_window=5, capacity=5):
    """The host statement of the selection (lsa_place_select_host): distance / shift the table of the frames 0..query-1,
    poses (n, 4, 4) and times (n,) as Slam.trajectory() gives them -> [(frame, distance, shift, yaw)], best first."""
    P = np.asarray(poses, np.float64).reshape(-1, 16)
    rows = np.ascontiguousarray(np.concatenate([P, np.asarray(times, np.float64).reshape(-1, 1)], axis=1))
    d = np.ascontiguousarray(np.asarray(distance, np.float32).reshape(-1))
    s = np.ascontiguousarray(np.asarray(shift, np.int32).reshape(-1))
    if d.size < max(int(query), 0) or s.size < max(int(query), 0):
        raise _error("lsa_place_select_host", E_ARG, "a table shorter than the frames before query")
    out = (PlaceCandidateStruct * max(int(capacity), 1))()
    rc = lib().lsa_place_select_host(ptr(d) if d.size else None, ptr(s) if s.size else None, ptr(rows), rows.shape[0], int(query), int(sectors), float(min_travelled),
                                     float(max_distance), float(max_descriptor_distance), int(exclusion_half_window), out, int(capacity))
    if rc < 0:
        raise _error("lsa_place_select_host", rc, "bad argument")
    return _candidates(out, rc)


# lsa_pgo_edge_t as a numpy record: from -> to, the measured inv(P[from]) @ P[to] (row-major 4x4), its 6x6 information
PGO_EDGE_DTYPE = np.dtype([("from", np.int32), ("to", np.int32), ("relative", np.float64, (16,)), ("information", np.float64, (36,))])
PGO_EDGE_BLOCK = 120  # doubles of an edge's block record: Haa[36] Hab[36] Hbb[36] ga[6] gb[6]
# lsa_pgo_prior_t: a measured position of the point carried by `pose` behind the solve's offset, and its 3x3 information
PGO_PRIOR_DTYPE = np.dtype([("pose", np.int32), ("reserved", np.int32), ("position", np.float64, (3,)), ("information", np.float64, (9,))])
PGO_PRIOR_BLOCK = 42  # doubles of a prior's block record: Haa[36] ga[6]
PGO_MAX_ITERATIONS, PGO_GRADIENT, PGO_STEP, PGO_COST, PGO_LAMBDA_CEILING, PGO_LINEAR_SOLVER_FAILED = range(6)


class PoseGraphParams(C.Structure):
    """lsa_pgo_params_t (include/lidarslam_amd.h); the defaults are lsa_pgo_params_init's."""

    _fields_ = [
        ("max_iterations", C.c_int32), ("pcg_max_iter", C.c_int32), ("preconditioner", C.c_int32), ("apply", C.c_int32), ("odometry_information", C.c_int32),
        ("reserved", C.c_int32), ("pcg_tolerance", C.c_double), ("initial_lambda", C.c_double), ("lambda_shrink", C.c_double), ("lambda_grow", C.c_double),
        ("lambda_min", C.c_double), ("lambda_max", C.c_double), ("gradient_tolerance", C.c_double), ("step_tolerance", C.c_double), ("cost_tolerance", C.c_double),
        ("odometry_sigma", C.c_double * 6),
    ]

    def __init__(self, **kw):
        super().__init__()
        lib().lsa_pgo_params_init(C.byref(self))
        for k, v in kw.items():
            if k == "odometry_sigma":
                v = (C.c_double * 6)(*[float(a) for a in v])
            elif k not in dict(self._fields_):
                raise TypeError(f"PoseGraphParams has no field {k!r}")
            setattr(self, k, v)


class PoseGraphResultStruct(C.Structure):
    """lsa_pgo_result_t."""

    _fields_ = [
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("largest_step", C.c_double), ("final_lambda", C.c_double),
        ("iterations", C.c_int32), ("accepted_steps", C.c_int32), ("rejected_steps", C.c_int32), ("pcg_iterations", C.c_int32),
        ("last_pcg_iterations", C.c_int32), ("pcg_truncated", C.c_int32), ("termination", C.c_int32), ("reserved", C.c_int32), ("message", C.c_char_p),
    ]


class PoseGraphResult:
    """What a pose-graph solve reports: initial_cost / final_cost (1/2 sum chi2), largest_step, final_lambda, iterations,
    accepted_steps, rejected_steps, pcg_iterations, last_pcg_iterations, pcg_truncated, termination (PGO_*), message."""

    def __init__(self, r):
        for name, _ in PoseGraphResultStruct._fields_:
            if name != "reserved":
                setattr(self, name, getattr(r, name))
        self.message = (r.message or b"").decode()

    def __repr__(self):
        return f"PoseGraphResult({self.__dict__})"


def pose_graph_edges(edges):
    """A PGO_EDGE_DTYPE array from one, or from an iterable of (from, to, relative (4, 4), information (6, 6))."""
    if isinstance(edges, np.ndarray) and edges.dtype == PGO_EDGE_DTYPE:
        return np.ascontiguousarray(edges)
    edges = list(edges)
    out = np.zeros(len(edges), PGO_EDGE_DTYPE)
    for k, (a, b, Z, W) in enumerate(edges):
        out[k]["from"], out[k]["to"] = int(a), int(b)
        out[k]["relative"] = np.asarray(Z, np.float64).reshape(16)
        out[k]["information"] = np.asarray(W, np.float64).reshape(36)
    return out


def pose_graph_priors(priors):
    """A PGO_PRIOR_DTYPE array from one, or from an iterable of (pose, position (3,), information (3, 3)); None: no prior."""
    if isinstance(priors, np.ndarray) and priors.dtype == PGO_PRIOR_DTYPE:
        return np.ascontiguousarray(priors)
    priors = [] if priors is None else list(priors)
    out = np.zeros(len(priors), PGO_PRIOR_DTYPE)
    for k, (i, g, W) in enumerate(priors):
        out[k]["pose"] = int(i)
        out[k]["position"] = np.asarray(g, np.float64).reshape(3)
        out[k]["information"] = np.asarray(W, np.float64).reshape(9)
    return out


def _pgo_graph(poses, fixed, edges):
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    E = pose_graph_edges(edges)
    f = None if fixed is None else np.ascontiguousarray(np.asarray(fixed).astype(np.uint8).reshape(-1))
    if f is not None and f.size != P.shape[0]:
        raise _error("pose graph", E_ARG, "as many fixed flags as poses")
    return P, f, E


def _pgo_priors(priors, offset):
    """-> the arguments (priors, k, offset16) of a lsa_pgo_*_priors call and the arrays they point into"""
    R = pose_graph_priors(priors)
    O = np.ascontiguousarray(np.asarray(np.eye(4) if offset is None else offset, np.float64).reshape(16))
    return [ptr(R) if R.size else None, R.size, ptr(O)], (R, O)


def _pgo_run(what, ctx, poses, fixed, edges, make_out, *extra, priors=None, offset=None):
    """One of the lsa_pgo_* calls that take (poses, n, [fixed,] edges, m, extra..., outputs...); ctx None: the _host twin.
    With priors the call is its _priors form, which takes (priors, k, offset16) behind the edges."""
    P, f, E = _pgo_graph(poses, fixed, edges)
    L = lib()
    pa, keep = ([], None) if priors is None else _pgo_priors(priors, offset)
    if priors is not None:
        what += "_priors"
    fn = getattr(L, what if ctx is not None else what + "_host")
    outs = make_out(P.shape[0], E.size)
    args = ([ctx.h] if ctx is not None else []) + [ptr(P), P.shape[0]] + ([] if f is None else [ptr(f)]) + [ptr(E) if E.size else None, E.size] + pa
    rc = fn(*args, *extra, *[ptr(o) if isinstance(o, np.ndarray) else o for o in outs])
    if rc < 0:
        raise _error(fn.__name__, rc, L.lsa_last_error(ctx.h).decode() if ctx is not None else "the graph is outside the definition")
    return outs


def pose_graph_solve(poses, fixed, edges, ctx=None, params=None, priors=None, offset=None, **kw):
    """Levenberg-Marquardt on the pose graph (lidarslam_amd/csrc/lsa_pose_graph.h): poses (n, 4, 4), fixed (n,) flags, edges as
    pose_graph_edges takes them -> (poses (n, 4, 4), PoseGraphResult).  ctx None: the host statement (lsa_pgo_solve_host); a
    Context: the device solver (lsa_pgo_solve).  params: a PoseGraphParams, or its fields as keywords.  priors: position
    priors as pose_graph_priors takes them, behind the (4, 4) offset (None: the identity) -- lsa_pgo_solve_priors[_host]."""
    p = params if params is not None else PoseGraphParams(**kw)
    r = PoseGraphResultStruct()
    P, f, E = _pgo_graph(poses, fixed, edges)
    if f is None:
        raise _error("lsa_pgo_solve", E_ARG, "fixed flags are needed")
    out = np.zeros((P.shape[0], 4, 4))
    L = lib()
    name = "lsa_pgo_solve" + ("" if priors is None else "_priors") + ("_host" if ctx is None else "")
    pa, keep = ([], None) if priors is None else _pgo_priors(priors, offset)
    args = ([] if ctx is None else [ctx.h]) + [ptr(P), P.shape[0], ptr(f), ptr(E) if E.size else None, E.size] + pa + [C.byref(p), ptr(out), C.byref(r)]
    rc = getattr(L, name)(*args)
    if rc < 0:
        raise _error(name, rc, "the graph or the parameters are outside the definition" if ctx is None else L.lsa_last_error(ctx.h).decode())
    return out, PoseGraphResult(r)


def pose_graph_solve_host(poses, fixed, edges, params=None, priors=None, offset=None, **kw):
    """pose_graph_solve without a device."""
    return pose_graph_solve(poses, fixed, edges, None, params, priors, offset, **kw)


def pose_graph_linearize(poses, edges, ctx=None):
    """-> e (m, 6), blocks (m, 120), chi2 (m,): k_pgo_linearize with a Context, its host twin without."""
    e, b, c = _pgo_run("lsa_pgo_linearize", ctx, poses, None, edges, lambda n, m: [np.zeros((m, 6)), np.zeros((m, PGO_EDGE_BLOCK)), np.zeros(m)])
    return e, b, c


def pose_graph_linearize_priors(poses, priors, offset=None, ctx=None):
    """-> e (k, 3), blocks (k, 42), chi2 (k,) of the position priors: k_pgo_linearize_priors with a Context, its host twin without."""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    pa, keep = _pgo_priors(priors, offset)
    k = pa[1]
    e, b, c = np.zeros((k, 3)), np.zeros((k, PGO_PRIOR_BLOCK)), np.zeros(k)
    L = lib()
    if ctx is None:
        rc = L.lsa_pgo_linearize_priors_host(ptr(P), P.shape[0], *pa, ptr(e), ptr(b), ptr(c))
    else:
        rc = L.lsa_pgo_linearize_priors(ctx.h, ptr(P), P.shape[0], *pa, ptr(e), ptr(b), ptr(c))
    if rc < 0:
        raise _error("lsa_pgo_linearize_priors", rc, L.lsa_last_error(ctx.h).decode() if ctx is not None else "a prior is outside the definition")
    return e, b, c


def pose_graph_prior_jacobian(poses, prior, offset=None):
    """e (3,) and A = de/ddelta (3, 6) of one prior (pose, position, information); the host statement."""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    pa, keep = _pgo_priors([prior] if isinstance(prior, tuple) else prior, offset)
    e, A = np.zeros(3), np.zeros((3, 6))
    rc = lib().lsa_pgo_prior_jacobian_host(ptr(P), P.shape[0], pa[0], pa[2], ptr(e), ptr(A))
    if rc < 0:
        raise _error("lsa_pgo_prior_jacobian_host", rc, "the prior is outside the definition")
    return e, A


def pose_graph_assemble(poses, fixed, edges, lam=0.0, ctx=None, priors=None, offset=None):
    """-> D (n, 6, 6) damped by lam, g (n, 6), L (n, 6, 6) = block (i, i-1), U (n, 6, 6) = block (i, i+1)."""
    D, g, Lo, U = _pgo_run("lsa_pgo_assemble", ctx, poses, fixed, edges, lambda n, m: [np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))],
                           C.c_double(lam), priors=priors, offset=offset)
    return D, g, Lo, U


def pose_graph_spmv(poses, fixed, edges, lam, p, ctx=None, priors=None, offset=None):
    """q = H_lambda p (n, 6), the blocks beyond the chain included."""
    pv = np.ascontiguousarray(np.asarray(p, np.float64).reshape(-1, 6))
    if pv.shape[0] != np.asarray(poses).reshape(-1, 16).shape[0]:
        raise _error("lsa_pgo_spmv", E_ARG, "a vector of another length than the poses")
    q, = _pgo_run("lsa_pgo_spmv", ctx, poses, fixed, edges, lambda n, m: [np.zeros((n, 6))], C.c_double(lam), ptr(pv), priors=priors, offset=offset)
    return q


def pose_graph_premultiply(poses, W, ctx=None):
    """W @ poses[i] for every pose (k_pgo_premultiply with a Context, its host twin without)."""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    Wm = np.ascontiguousarray(np.asarray(W, np.float64).reshape(16))
    out = np.zeros((P.shape[0], 4, 4))
    lb = lib()
    rc = lb.lsa_pgo_premultiply_host(ptr(P), P.shape[0], ptr(Wm), ptr(out)) if ctx is None else lb.lsa_pgo_premultiply(ctx.h, ptr(P), P.shape[0], ptr(Wm), ptr(out))
    if rc < 0:
        raise _error("lsa_pgo_premultiply", rc, lb.lsa_last_error(ctx.h).decode() if ctx is not None else "bad argument")
    return out


def pose_graph_reanchor(poses, ctx=None):
    """inv(poses[0]) @ poses[i] for every pose (k_pgo_reanchor with a Context, its host twin without)."""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    out = np.zeros((P.shape[0], 4, 4))
    lb = lib()
    rc = lb.lsa_pgo_reanchor_host(ptr(P), P.shape[0], ptr(out)) if ctx is None else lb.lsa_pgo_reanchor(ctx.h, ptr(P), P.shape[0], ptr(out))
    if rc < 0:
        raise _error("lsa_pgo_reanchor", rc, lb.lsa_last_error(ctx.h).decode() if ctx is not None else "bad argument")
    return out


def pose_graph_tridiagonal_solve(D, L, U, b, ctx=None):
    """x (n, 6) with T x = b for the block-tridiagonal T = (D, L, U), each (n, 6, 6): cyclic reduction on the device with a
    Context, block Thomas on the host without.  None when a block is not positive definite."""
    D, L, U = [np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 36)) for a in (D, L, U)]
    b = np.ascontiguousarray(np.asarray(b, np.float64).reshape(-1, 6))
    n = D.shape[0]
    if not (L.shape[0] == U.shape[0] == b.shape[0] == n):
        raise _error("lsa_pgo_tridiagonal_solve", E_ARG, "arrays of different lengths")
    x = np.full((n, 6), np.nan)
    lb = lib()
    if ctx is None:
        rc = lb.lsa_pgo_tridiagonal_solve_host(n, ptr(D), ptr(L), ptr(U), ptr(b), ptr(x))
    else:
        rc = lb.lsa_pgo_tridiagonal_solve(ctx.h, n, ptr(D), ptr(L), ptr(U), ptr(b), ptr(x))
    if rc < 0:
        raise _error("lsa_pgo_tridiagonal_solve", rc, lb.lsa_last_error(ctx.h).decode() if ctx is not None else "bad argument")
    return None if rc == 1 else x


def pose_graph_retract(poses, delta, ctx=None):
    """poses (n, 4, 4) moved by delta (n, 6) = (rho, phi): t += R rho, R = R Exp(phi) (k_pgo_retract with a Context)."""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    d = np.ascontiguousarray(np.asarray(delta, np.float64).reshape(-1, 6))
    if d.shape[0] != P.shape[0]:
        raise _error("lsa_pgo_retract", E_ARG, "as many steps as poses")
    out = np.zeros((P.shape[0], 4, 4))
    lb = lib()
    rc = lb.lsa_pgo_retract_host(ptr(P), P.shape[0], ptr(d), ptr(out)) if ctx is None else lb.lsa_pgo_retract(ctx.h, ptr(P), P.shape[0], ptr(d), ptr(out))
    if rc < 0:
        raise _error("lsa_pgo_retract", rc, lb.lsa_last_error(ctx.h).decode() if ctx is not None else "bad argument")
    return out


def pose_graph_edge_jacobians(poses, edge):
    """e (6,), A = de/ddelta_from (6, 6), B = de/ddelta_to (6, 6) of one edge; the host statement."""
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    E = pose_graph_edges([edge] if isinstance(edge, tuple) else edge)
    e, A, B = np.zeros(6), np.zeros((6, 6)), np.zeros((6, 6))
    rc = lib().lsa_pgo_edge_jacobians_host(ptr(P), P.shape[0], ptr(E), ptr(e), ptr(A), ptr(B))
    if rc < 0:
        raise _error("lsa_pgo_edge_jacobians_host", rc, "the edge is outside the definition")
    return e, A, B


def information_from_covariance(cov):
    """The inverse of a symmetric positive definite 6x6 (lsa_pgo_information_from_covariance); raises for anything else."""
    c = np.ascontiguousarray(np.asarray(cov, np.float64).reshape(36))
    out = np.zeros((6, 6))
    rc = lib().lsa_pgo_information_from_covariance(ptr(c), ptr(out))
    if rc < 0:
        raise _error("lsa_pgo_information_from_covariance", rc, "not a symmetric positive definite matrix")
    return out


def information_from_covariance3(cov):
    """The inverse of a symmetric positive definite 3x3 (lsa_pgo_information_from_covariance3); raises for anything else."""
    c = np.ascontiguousarray(np.asarray(cov, np.float64).reshape(9))
    out = np.zeros((3, 3))
    rc = lib().lsa_pgo_information_from_covariance3(ptr(c), ptr(out))
    if rc < 0:
        raise _error("lsa_pgo_information_from_covariance3", rc, "not a symmetric positive definite matrix")
    return out


def gps_match_trajectory(slam_times, gps_times, time_offset=0.0, max_time_diff=0.1):
    """Per GPS fix the index of the logged pose (dated slam_times + time_offset) nearest in time within max_time_diff, the
    earlier of two equally near; -1 for none and for a fix whose pose the fix accepted before it already took
    (lsa_gps_match_trajectory).  Times ascending."""
    s = np.ascontiguousarray(np.asarray(slam_times, np.float64).reshape(-1))
    g = np.ascontiguousarray(np.asarray(gps_times, np.float64).reshape(-1))
    out = np.full(g.size, -2, np.int32)
    rc = lib().lsa_gps_match_trajectory(ptr(s) if s.size else None, s.size, ptr(g) if g.size else None, g.size, float(time_offset), float(max_time_diff),
                                        ptr(out) if g.size else None)
    if rc < 0:
        raise _error("lsa_gps_match_trajectory", rc, "times that are not finite and ascending, or a negative bound")
    return out


def trajectory_alignment(from_xyz, to_xyz):
    """The rigid (4, 4) T minimising sum |T from_i - to_i|^2 over the pairs (Horn's closed form; the reference's rough
    estimate for fewer than three pairs or collinear tracks) -- lsa_trajectory_alignment."""
    a = np.ascontiguousarray(np.asarray(from_xyz, np.float64).reshape(-1, 3))
    b = np.ascontiguousarray(np.asarray(to_xyz, np.float64).reshape(-1, 3))
    if a.shape != b.shape:
        raise _error("lsa_trajectory_alignment", E_ARG, "as many points from as to")
    T = np.zeros((4, 4))
    rc = lib().lsa_trajectory_alignment(ptr(a) if a.size else None, ptr(b) if b.size else None, a.shape[0], ptr(T))
    if rc < 0:
        raise _error("lsa_trajectory_alignment", rc, "no pair, or a non-finite coordinate")
    return T


class SensorTerms(C.Structure):
    """lsa_sensor_terms_t (include/lidarslam_amd.h): the wheel odometer and gravity terms of the localization problem.
    ``SensorTerms(wheel_weight=1.0, d=3.0)`` turns the odometer term on, ``gravity_weight=...`` the gravity term."""

    _fields_ = [
        ("wheel", C.c_int), ("wheel_weight", C.c_double), ("p", C.c_double * 3), ("d", C.c_double),
        ("gravity", C.c_int), ("gravity_weight", C.c_double), ("g_ref", C.c_double * 3), ("g_cur", C.c_double * 3),
    ]

    def __init__(self, wheel_weight=None, p=(0.0, 0.0, 0.0), d=0.0, gravity_weight=None, g_ref=(0.0, 0.0, 1.0), g_cur=(0.0, 0.0, 1.0)):
        super().__init__()
        if wheel_weight is not None:
            self.wheel, self.wheel_weight, self.d = 1, float(wheel_weight), float(d)
            self.p[:] = [float(v) for v in p]
        if gravity_weight is not None:
            self.gravity, self.gravity_weight = 1, float(gravity_weight)
            self.g_ref[:] = [float(v) for v in g_ref]
            self.g_cur[:] = [float(v) for v in g_cur]

    def as_tuple(self):
        """every field, in order (the flags as ints): equal tuples are equal terms, bit for bit"""
        return (self.wheel, self.wheel_weight, *self.p, self.d, self.gravity, self.gravity_weight, *self.g_ref, *self.g_cur)


def sensor_terms_eval(terms, w):
    """lsa_sensor_terms_eval: the terms' 29 sums (cost, g[6], H upper triangle, count) at w, on the host (libm)"""
    w = np.ascontiguousarray(w, np.float64)
    out = np.zeros(29)
    if lib().lsa_sensor_terms_eval(C.byref(terms), ptr(w), ptr(out)) != 0:
        raise LsaError("lsa_sensor_terms_eval")
    return out


def sums_to_normal_equations(sums):
    """29 sums -> (cost, g[6], H 6x6, count)"""
    g = np.array(sums[1:7])
    H = np.zeros((6, 6))
    h = 7
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = sums[h]
            h += 1
    return float(sums[0]), g, H, int(sums[28])


class Sensors:
    """The wheel odometer / IMU managers of LidarSlam::Slam without a device (lsa_sensors_*)."""

    def __init__(self):
        self.L = lib()
        self.h = self.L.lsa_sensors_create()

    def close(self):
        if getattr(self, "h", None):
            self.L.lsa_sensors_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def add_wheel_odom(self, time, distance):
        self.L.lsa_sensors_add_wheel_odom(self.h, float(time), float(distance))

    def add_gravity(self, time, acc):
        a = np.ascontiguousarray(acc, np.float64)
        self.L.lsa_sensors_add_gravity(self.h, float(time), ptr(a))

    def set_weights(self, wheel, gravity):
        self.L.lsa_sensors_set_weights(self.h, float(wheel), float(gravity))

    def set_time_offset(self, offset):
        self.L.lsa_sensors_set_time_offset(self.h, float(offset))

    def clear(self):
        self.L.lsa_sensors_clear(self.h)

    def compute(self, lidar_time):
        t = SensorTerms()
        self.L.lsa_sensors_compute(self.h, float(lidar_time), C.byref(t))
        return t

    def gravity_ref(self):
        g = np.zeros(3)
        have = self.L.lsa_sensors_gravity_ref(self.h, ptr(g))
        return g, bool(have)


def icp_link_expected(x6, skipped, successful_steps, link):
    """lsa_icp_link_expected: (the 64 words of the block, the motion afterwards) as the host's arithmetic gives them"""
    words, motion = np.zeros(64, np.uint64), np.zeros(16, np.float64)
    x = np.ascontiguousarray(x6, np.float64)
    L = lib()
    L.lsa_icp_link_expected.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    if L.lsa_icp_link_expected(ptr(x), int(skipped), int(successful_steps), C.byref(link), ptr(words), ptr(motion)) != 0:
        raise LsaError("lsa_icp_link_expected")
    return words, motion


# lsa_selftest_numerics: (doubles per input record, per output record) by fn (include/lidarslam_amd.h)
NUMERICS_FNS = {"PCA_F": 0, "PCA_D": 1, "EIG33_F": 2, "EIG33_D": 3, "SPD3": 4, "SPD6": 5, "ACCUM": 6, "POSE": 7,
                "SPD3_HOST": 8, "SPD6_HOST": 9, "JACOBI3_HOST": 10, "JACOBI6_HOST": 11}
NUMERICS_WIDTHS = [(49, 15), (49, 15), (6, 12), (6, 12), (12, 4), (42, 7), (23, 28), (42, 39), (12, 4), (42, 7), (9, 12), (36, 42)]


def selftest_numerics(fn, records, ctx=None):
    """lsa_selftest_numerics: records (n, IN) -> (n, OUT).  fn 0-7 need a Context (the device), fn 8-11 run the
    host twins on the CPU and need none."""
    win, wout = NUMERICS_WIDTHS[fn]
    rec = np.ascontiguousarray(records, np.float64).reshape(-1, win)
    out = np.zeros((rec.shape[0], wout))
    L = lib()
    rc = L.lsa_selftest_numerics(ctx.h if ctx is not None else None, int(fn), ptr(rec), rec.shape[0], ptr(out))
    if rc < 0:
        raise LsaError(f"lsa_selftest_numerics({fn}) failed ({rc})" + (f": {L.lsa_last_error(ctx.h).decode()}" if ctx is not None else ""))
    return out


_lib = None


def lib():
    """Loads liblidarslam_amd.so (built in-tree by __graft_entry__.build()); raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LsaError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(LIB_PATH)
    vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
    L.lsa_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.lsa_ctx_destroy.argtypes = [vp]
    L.lsa_last_error.restype = C.c_char_p
    L.lsa_last_error.argtypes = [vp]
    L.lsa_sync.argtypes = [vp]
    L.lsa_upload_frame.argtypes = [vp, vp, i32]
    L.lsa_frame_store_put.argtypes = [vp, i32, vp, i32]
    L.lsa_frame_store_use.argtypes = [vp, i32]
    L.lsa_frame_size.argtypes = [vp]
    L.lsa_get_azimuthal_resolution.restype = C.c_float
    L.lsa_get_azimuthal_resolution.argtypes = [vp]
    L.lsa_set_azimuthal_resolution.argtypes = [vp, C.c_float]
    L.lsa_extract_keypoints.argtypes = [vp, C.POINTER(ExtractParams), vp]
    L.lsa_download_keypoints.argtypes = [vp, i32, i32, vp, i32]
    L.lsa_keypoint_count.argtypes = [vp, i32, i32]
    L.lsa_download_debug.argtypes = [vp, i32, vp, i32]
    L.lsa_nb_laser_rings.argtypes = [vp]
    L.lsa_transform_keypoints.argtypes = [vp, i32, i32, vp, f64]
    L.lsa_set_target.argtypes = [vp, i32, i32, vp, i32]
    L.lsa_set_target_from_set.argtypes = [vp, i32, i32, i32]
    L.lsa_target_size.argtypes = [vp, i32, i32]
    L.lsa_set_target_cell_size.argtypes = [vp, i32, i32, C.c_float]
    L.lsa_match_slow_queries.argtypes = [vp]
    L.lsa_set_keypoints.argtypes = [vp, i32, i32, vp, i32]
    L.lsa_match.argtypes = [vp, i32, i32, i32, C.POINTER(MatchParams), vp, vp]
    L.lsa_set_knn_lanes.argtypes = [vp, i32, i32]
    L.lsa_set_fused_match.argtypes = [vp, i32]
    L.lsa_overlap.argtypes = [vp, C.c_uint, i32, vp, vp, C.c_double, C.c_double, C.c_float, vp, vp]
    L.lsa_upload_wire_frame.argtypes = [vp, vp, i32, vp, vp, i32, i32, C.c_double, i32]
    L.lsa_match_types.argtypes = [vp, i32, C.c_uint, i32, C.POINTER(MatchParams), vp, vp]
    L.lsa_match_types_undistorted.argtypes = [vp, i32, C.c_uint, C.POINTER(MatchParams), vp, vp, vp, vp, f64, f64]
    L.lsa_download_match.argtypes = [vp, i32, vp, vp, vp, i32]
    L.lsa_upload_match.argtypes = [vp, i32, vp, vp, i32, f64]
    L.lsa_download_knn.argtypes = [vp, i32, vp, vp, vp, i32]
    L.lsa_accumulate.argtypes = [vp, C.c_uint, vp, i32, vp, vp, vp, vp]
    L.lsa_solve.argtypes = [vp, C.c_uint, vp, i32, i32, vp, vp, vp]
    L.lsa_registration_error.argtypes = [vp, C.c_uint, vp, i32, vp, vp]
    L.lsa_solve_device.argtypes = [vp, C.c_uint, vp, i32, i32, i32, C.POINTER(SolveResult)]
    L.lsa_solve_device_fallbacks.argtypes = [vp]
    L.lsa_solve_device_shape.argtypes = [vp, vp]
    L.lsa_accumulate_shape.argtypes = [vp, vp]
    L.lsa_selftest_math.argtypes = [vp, i32, vp, vp, i32, vp]
    L.lsa_selftest_numerics.argtypes = [vp, i32, vp, i32, vp]
    L.lsa_selftest_labels.argtypes = [vp, C.POINTER(ExtractParams), vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.lsa_reset_working_keypoints.argtypes = [vp]
    L.lsa_undistort.argtypes = [vp, vp, vp, f64, f64]
    L.lsa_working_time_range.argtypes = [vp, vp, vp]
    L.lsa_keypoint_time_range.argtypes = [vp, i32, vp, vp]
    L.lsa_keypoint_bboxes_begin.argtypes = [vp, i32, vp]
    L.lsa_localization_begin.argtypes = [vp, vp, vp, f64, f64, vp]
    L.lsa_arm_localization_boxes.argtypes = [vp]
    L.lsa_keypoint_bboxes_begin_interp.argtypes = [vp, i32, vp, vp, f64, f64]
    L.lsa_keypoint_bboxes_end.argtypes = [vp, vp, vp]
    L.lsa_keypoint_boxes_predicted_mark.argtypes = [vp]
    L.lsa_keypoint_boxes_predicted.argtypes = [vp, i32, vp, vp, f64, f64]
    L.lsa_working_bbox.argtypes = [vp, i32, vp, vp, vp]
    L.lsa_download_transformed.argtypes = [vp, i32, i32, vp, vp, i32]
    L.lsa_transform_frame.argtypes = [vp, i32, vp, vp, f64, f64, vp, i32]
    L.lsa_profile_enable.argtypes = [vp, i32]
    L.lsa_profile_select.argtypes = [vp, C.c_char_p, i32]
    L.lsa_profile_reset.argtypes = [vp]
    L.lsa_profile_get.argtypes = [vp, vp, i32]
    L.lsa_slam_create.argtypes = [i32, C.POINTER(vp)]
    L.lsa_slam_destroy.argtypes = [vp]
    L.lsa_slam_last_error.restype = C.c_char_p
    L.lsa_slam_last_error.argtypes = [vp]
    L.lsa_slam_set_param.argtypes = [vp, C.c_char_p, f64]
    L.lsa_slam_get_param.argtypes = [vp, C.c_char_p, vp]
    L.lsa_slam_reset.argtypes = [vp, i32]
    L.lsa_slam_add_frame.argtypes = [vp, vp, i32, C.c_uint64, C.c_uint32]
    L.lsa_slam_store_frame.argtypes = [vp, i32, vp, i32]
    L.lsa_slam_add_stored_frame.argtypes = [vp, i32, C.c_uint64, C.c_uint32]
    L.lsa_slam_get_world_transform.argtypes = [vp, vp, vp]
    L.lsa_slam_get_covariance.argtypes = [vp, vp]
    L.lsa_slam_get_keypoints.argtypes = [vp, i32, i32, vp, i32]
    L.lsa_slam_get_registered_frame.argtypes = [vp, vp, i32]
    L.lsa_slam_get_match_status.argtypes = [vp, i32, i32, vp, vp, i32]
    L.lsa_slam_get_stats.argtypes = [vp, vp]
    L.lsa_slam_context.restype = vp
    L.lsa_slam_context.argtypes = [vp]
    L.lsa_slam_get_latency_compensated_world_transform.argtypes = [vp, vp, vp]
    L.lsa_slam_set_world_transform_from_guess.argtypes = [vp, vp]
    L.lsa_slam_get_trajectory.argtypes = [vp, vp, vp, i32]
    L.lsa_slam_hint_next_stored_frame.argtypes = [vp, i32]
    L.lsa_slam_hint_next_frame.argtypes = [vp, vp, i32]
    L.lsa_upload_frame_begin.argtypes = [vp, vp, i32]
    L.lsa_upload_frame_ready.argtypes = [vp]
    L.lsa_upload_frame_adopt.argtypes = [vp, vp, i32]
    L.lsa_uploads_adopted.argtypes = [vp]
    L.lsa_extract_prefetch_uploaded.argtypes = [vp, C.POINTER(ExtractParams)]
    L.lsa_slam_add_frames.argtypes = [vp, vp, vp, vp, vp, i32]
    L.lsa_slam_set_extractor_param.argtypes = [vp, i32, C.c_char_p, f64]
    L.lsa_slam_get_extractor_param.argtypes = [vp, i32, C.c_char_p, vp]
    L.lsa_slam_set_base_to_lidar_offset.argtypes = [vp, vp, i32]
    L.lsa_slam_get_base_to_lidar_offset.argtypes = [vp, vp, i32]
    L.lsa_slam_get_debug_information.argtypes = [vp, vp]
    L.lsa_slam_get_map.argtypes = [vp, i32, i32, vp, i32]
    L.lsa_slam_get_target_submap.argtypes = [vp, i32, vp, i32]
    L.lsa_match_serial.restype = C.c_longlong
    L.lsa_match_serial.argtypes = [vp, i32]
    L.lsa_match_histogram.argtypes = [vp, i32, C.c_longlong, vp]
    L.lsa_rolling_grid_create.restype = vp
    L.lsa_rolling_grid_create.argtypes = []
    L.lsa_rolling_grid_destroy.argtypes = [vp]
    L.lsa_rolling_grid_destroy.restype = None
    L.lsa_rolling_grid_set.argtypes = [vp, C.c_char_p, f64]
    L.lsa_rolling_grid_reset.argtypes = [vp, vp]
    L.lsa_rolling_grid_reset.restype = None
    L.lsa_rolling_grid_clear.argtypes = [vp]
    L.lsa_rolling_grid_clear.restype = None
    L.lsa_rolling_grid_size.argtypes = [vp]
    L.lsa_rolling_grid_roll.argtypes = [vp, vp, vp]
    L.lsa_rolling_grid_roll.restype = None
    L.lsa_rolling_grid_add.argtypes = [vp, vp, i32, i32, f64, i32]
    L.lsa_rolling_grid_clear_old_points.argtypes = [vp, f64]
    L.lsa_rolling_grid_clear_old_points.restype = None
    L.lsa_rolling_grid_get.argtypes = [vp, i32, vp, i32]
    L.lsa_rolling_grid_build_submap.argtypes = [vp, vp, vp, i32]
    L.lsa_rolling_grid_submap_valid.argtypes = [vp]
    L.lsa_rolling_grid_submap.argtypes = [vp, vp, i32]
    L.lsa_set_sensor_terms.argtypes = [vp, vp]
    L.lsa_sensor_terms_eval.argtypes = [vp, vp, vp]
    L.lsa_sensors_create.restype = vp
    L.lsa_sensors_create.argtypes = []
    L.lsa_sensors_destroy.restype = None
    L.lsa_sensors_destroy.argtypes = [vp]
    L.lsa_sensors_add_wheel_odom.argtypes = [vp, f64, f64]
    L.lsa_sensors_add_gravity.argtypes = [vp, f64, vp]
    L.lsa_sensors_set_weights.argtypes = [vp, f64, f64]
    L.lsa_sensors_set_time_offset.argtypes = [vp, f64]
    L.lsa_sensors_clear.argtypes = [vp]
    L.lsa_sensors_compute.argtypes = [vp, f64, vp]
    L.lsa_sensors_gravity_ref.argtypes = [vp, vp]
    L.lsa_slam_add_wheel_odom_measurement.argtypes = [vp, f64, f64]
    L.lsa_slam_add_gravity_measurement.argtypes = [vp, f64, vp]
    L.lsa_slam_clear_sensor_measurements.argtypes = [vp]
    L.lsa_slam_sensor_terms.argtypes = [vp, vp]
    L.lsa_pcd_info.argtypes = [C.c_char_p, C.POINTER(i32), C.POINTER(i32)]
    L.lsa_pcd_read.argtypes = [C.c_char_p, vp, i32]
    L.lsa_pcd_write.argtypes = [C.c_char_p, vp, i32, i32]
    L.lsa_pcd_last_error.restype = C.c_char_p
    L.lsa_pcd_last_error.argtypes = []
    L.lsa_lzf_compress.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lsa_lzf_decompress.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.lsa_device_grid_add_pcd.argtypes = [vp, C.c_char_p, i32, f64, i32]
    L.lsa_device_grid_save_pcd.argtypes = [vp, C.c_char_p, i32, i32]
    L.lsa_pcd_io_times.argtypes = [vp, vp]
    L.lsa_slam_add_map_points.argtypes = [vp, i32, vp, i32, i32, f64]
    L.lsa_slam_save_maps_pcd.argtypes = [vp, C.c_char_p, i32, i32]
    L.lsa_slam_load_maps_pcd.argtypes = [vp, C.c_char_p, i32, f64]
    L.lsa_slam_map_io_counts.argtypes = [vp, vp]
    L.lsa_kplog_append.argtypes = [vp]
    L.lsa_kplog_append_points.argtypes = [vp, vp, vp]
    L.lsa_kplog_pop_front.argtypes = [vp]
    L.lsa_kplog_clear.argtypes = [vp]
    L.lsa_kplog_size.argtypes = [vp]
    L.lsa_kplog_count.argtypes = [vp, i32, i32]
    L.lsa_kplog_get.argtypes = [vp, i32, i32, vp, i32]
    L.lsa_kplog_bytes.restype = C.c_ulonglong
    L.lsa_kplog_bytes.argtypes = [vp]
    L.lsa_kplog_stopped.argtypes = [vp]
    L.lsa_kplog_replay.argtypes = [vp, C.c_uint, vp, vp, i32, i32, vp, vp, vp]
    L.lsa_kplog_replayed.restype = C.c_longlong
    L.lsa_kplog_replayed.argtypes = [vp, i32, vp]
    L.lsa_kplog_replay_to_grids.argtypes = [vp, C.c_uint, vp, vp, i32, i32, vp, vp, vp]
    L.lsa_kplog_replay_range.argtypes = [vp, C.c_uint, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.lsa_loop_closure_params_init.restype = None
    L.lsa_loop_closure_params_init.argtypes = [vp]
    L.lsa_slam_register_logged_frames.argtypes = [vp, i32, i32, vp, vp, vp]
    L.lsa_loop_closure_candidate.argtypes = [vp, i32, i32, C.c_double, C.c_double]
    L.lsa_place_params_init.restype = None
    L.lsa_place_params_init.argtypes = [vp]
    L.lsa_place_search_init.restype = None
    L.lsa_place_search_init.argtypes = [vp]
    L.lsa_scan_descriptor_host.argtypes = [vp, vp, i32, vp]
    L.lsa_place_distance_host.argtypes = [vp, vp, vp, vp, vp]
    L.lsa_place_select_host.argtypes = [vp, vp, vp, i32, i32, i32, C.c_double, C.c_double, C.c_double, i32, vp, i32]
    L.lsa_slam_recognize_place.argtypes = [vp, i32, vp, vp, i32]
    L.lsa_kplog_describe.argtypes = [vp, vp, i32, i32]
    L.lsa_kplog_descriptors.argtypes = [vp, i32, i32, vp]
    L.lsa_kplog_place_search.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    L.lsa_kplog_described.argtypes = [vp]
    L.lsa_kplog_descriptor_length.argtypes = [vp]
    L.lsa_pgo_params_init.restype = None
    L.lsa_pgo_params_init.argtypes = [vp]
    L.lsa_pgo_solve_host.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp]
    L.lsa_pgo_solve.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    L.lsa_pgo_linearize_host.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.lsa_pgo_linearize.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    L.lsa_pgo_assemble_host.argtypes = [vp, i32, vp, vp, i32, f64, vp, vp, vp, vp]
    L.lsa_pgo_assemble.argtypes = [vp, vp, i32, vp, vp, i32, f64, vp, vp, vp, vp]
    L.lsa_pgo_tridiagonal_solve_host.argtypes = [i32, vp, vp, vp, vp, vp]
    L.lsa_pgo_tridiagonal_solve.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.lsa_pgo_spmv_host.argtypes = [vp, i32, vp, vp, i32, f64, vp, vp]
    L.lsa_pgo_spmv.argtypes = [vp, vp, i32, vp, vp, i32, f64, vp, vp]
    L.lsa_pgo_information_from_covariance.argtypes = [vp, vp]
    L.lsa_pgo_retract_host.argtypes = [vp, i32, vp, vp]
    L.lsa_pgo_retract.argtypes = [vp, vp, i32, vp, vp]
    L.lsa_pgo_edge_jacobians_host.argtypes = [vp, i32, vp, vp, vp, vp]
    L.lsa_pgo_solve_priors_host.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
    L.lsa_pgo_solve_priors.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp]
    L.lsa_pgo_linearize_priors_host.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp]
    L.lsa_pgo_linearize_priors.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp]
    L.lsa_pgo_assemble_priors_host.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp, vp, vp]
    L.lsa_pgo_assemble_priors.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp, vp, vp]
    L.lsa_pgo_spmv_priors_host.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp]
    L.lsa_pgo_spmv_priors.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, f64, vp, vp]
    L.lsa_pgo_prior_jacobian_host.argtypes = [vp, i32, vp, vp, vp, vp]
    L.lsa_pgo_premultiply_host.argtypes = [vp, i32, vp, vp]
    L.lsa_pgo_premultiply.argtypes = [vp, vp, i32, vp, vp]
    L.lsa_pgo_reanchor_host.argtypes = [vp, i32, vp]
    L.lsa_pgo_reanchor.argtypes = [vp, vp, i32, vp]
    L.lsa_pgo_information_from_covariance3.argtypes = [vp, vp]
    L.lsa_gps_match_trajectory.argtypes = [vp, i32, vp, i32, f64, f64, vp]
    L.lsa_trajectory_alignment.argtypes = [vp, vp, i32, vp]
    L.lsa_slam_run_pose_graph_optimization.argtypes = [vp, vp, vp, vp, i32, vp, f64, vp, vp, i32, vp]
    L.lsa_slam_optimize_logged_trajectory.argtypes = [vp, vp, i32, vp, vp, i32, vp]
    L.lsa_slam_set_trajectory_and_rebuild_maps.argtypes = [vp, vp, i32]
    L.lsa_slam_logged_frames.argtypes = [vp]
    L.lsa_slam_get_logged_keypoints.argtypes = [vp, i32, i32, vp, i32]
    _lib = L
    return L


def _profile(L, h):
    buf = (KernelStat * 64)()
    n = L.lsa_profile_get(h, buf, 64)
    return [
        {"name": buf[i].name.decode(), "launches": buf[i].launches, "total_ms": buf[i].total_ms, "bytes": buf[i].bytes}
        for i in range(max(n, 0))
    ]


def pcd_info(path):
    """(number of points, format) of a PCD file; host only"""
    L = lib()
    n, fmt = C.c_int(), C.c_int()
    if L.lsa_pcd_info(os.fsencode(path), C.byref(n), C.byref(fmt)) != 0:
        raise LsaError(L.lsa_pcd_last_error().decode())
    return n.value, fmt.value


def read_pcd(path):
    """A PCD file as LidarPoints (POINT_DTYPE): any field order, missing fields 0, extra fields ignored; host only."""
    L = lib()
    n, _ = pcd_info(path)
    out = np.zeros(max(n, 1), POINT_DTYPE)
    got = L.lsa_pcd_read(os.fsencode(path), ptr(out), out.size)
    if got < 0:
        raise LsaError(L.lsa_pcd_last_error().decode())
    return out[:got].copy()


def write_pcd(path, pts, fmt=PCD_BINARY):
    """Writes LidarPoints as a PCD file (fmt: 0 ascii, 1 binary, 2 binary_compressed); host only.  Returns False, and
    writes nothing, for an empty cloud (savePointCloudToPCD's -3)."""
    L = lib()
    pts = np.ascontiguousarray(pts, POINT_DTYPE)
    rc = L.lsa_pcd_write(os.fsencode(path), ptr(pts) if pts.size else None, pts.size, int(fmt))
    if rc == -3 and pts.size == 0:
        return False
    if rc != 0:
        raise LsaError(f"lsa_pcd_write failed ({rc}): {L.lsa_pcd_last_error().decode()}")
    return True


def lzf_compress(data):
    L = lib()
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.zeros(src.size + src.size // 16 + 64, np.uint8)
    n = C.c_size_t()
    if L.lsa_lzf_compress(ptr(src) if src.size else None, src.size, ptr(out), out.size, C.byref(n)) != 0:
        raise LsaError("lsa_lzf_compress failed")
    return out[: n.value].tobytes()


def lzf_decompress(data, raw_size):
    L = lib()
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.zeros(max(raw_size, 1), np.uint8)
    n = C.c_size_t()
    if L.lsa_lzf_decompress(ptr(src) if src.size else None, src.size, ptr(out), raw_size, C.byref(n)) != 0:
        raise LsaError("lsa_lzf_decompress: malformed stream")
    return out[: n.value].tobytes()


def bind_host_to_device(device=0):
    """lsa_bind_host_to_device: keep this thread (and the ones created after) on the GPU's NUMA node; returns the
    node, or a negative code when there is nothing to bind to"""
    return lib().lsa_bind_host_to_device(int(device))


class Context:
    """Kernel-level operations of one device context (see include/lidarslam_amd.h)."""

    def __init__(self, device=0, handle=None):
        self.L = lib()
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            rc = self.L.lsa_ctx_create(device, C.byref(h))
            if rc != 0:
                raise LsaError(f"lsa_ctx_create({device}) failed with {rc}: no usable HIP device (no CPU fallback)")
            handle = h
        self.h = handle

    def close(self):
        if getattr(self, "h", None) and self._owned:
            self.L.lsa_ctx_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise _error(what, rc, self.L.lsa_last_error(self.h).decode())
        return rc

    # ---- frame / extraction
    def upload_frame(self, pts):
        pts = np.ascontiguousarray(pts)
        assert pts.dtype == POINT_DTYPE
        self._check(self.L.lsa_upload_frame(self.h, ptr(pts), pts.size), "lsa_upload_frame")

    def store_frame(self, slot, pts):
        pts = np.ascontiguousarray(pts)
        self._check(self.L.lsa_frame_store_put(self.h, slot, ptr(pts), pts.size), "lsa_frame_store_put")

    def use_stored_frame(self, slot):
        self._check(self.L.lsa_frame_store_use(self.h, slot), "lsa_frame_store_use")

    @property
    def azimuthal_resolution(self):
        return self.L.lsa_get_azimuthal_resolution(self.h)

    @azimuthal_resolution.setter
    def azimuthal_resolution(self, v):
        self.L.lsa_set_azimuthal_resolution(self.h, v)

    def upload_wire_frame(self, records, layout, mapping=None, device_id=0, rpm=600.0, timestamp_first_packet=False):
        """lsa_upload_wire_frame: records = contiguous structured / byte array of n driver records;
        layout = (point_step, off_x, off_y, off_z, off_intensity, off_ring, off_time)."""
        rec = np.ascontiguousarray(records)
        lay = (C.c_int32 * 7)(*[int(v) for v in layout])
        n = rec.nbytes // int(layout[0])
        mp = np.ascontiguousarray(mapping, np.uint16) if mapping is not None else None
        self._check(self.L.lsa_upload_wire_frame(self.h, rec.ctypes.data_as(C.c_void_p), n, lay, ptr(mp) if mp is not None else None,
                                                 0 if mp is None else mp.size, device_id, C.c_double(rpm), int(timestamp_first_packet)),
                    "lsa_upload_wire_frame")

    def upload_robosense_frame(self, records, width, height, layout, mapping=None, device_id=0, rpm=600.0):
        """lsa_upload_robosense_frame: the RoboSense driver's organized cloud (height lasers x width points) of records with
        float x, y, z, intensity; layout = (point_step, off_x, off_y, off_z, off_intensity).  Returns the points kept."""
        rec = np.ascontiguousarray(records)
        lay = (C.c_int32 * 7)(*([int(v) for v in layout] + [0, 0]))
        mp = np.ascontiguousarray(mapping, np.uint16) if mapping is not None else None
        kept = C.c_int()
        self.L.lsa_upload_robosense_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
        self._check(self.L.lsa_upload_robosense_frame(self.h, rec.ctypes.data_as(C.c_void_p), width, height, lay, ptr(mp) if mp is not None else None,
                                                      0 if mp is None else mp.size, device_id, rpm, C.byref(kept)), "lsa_upload_robosense_frame")
        return kept.value

    def upload_polydata_frame(self, xyz, time, laser_id, intensity, mapping=None, time_to_seconds=1.0):
        """lsa_upload_polydata_frame: the arrays of a vtkPolyData frame (xyz (n, 3) float32 / float64, the others any of
        float32, float64, uint8, uint16, uint32, int32); returns (stamp_us, points kept, all points valid)."""
        codes = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint8): 2, np.dtype(np.uint16): 3, np.dtype(np.uint32): 4, np.dtype(np.int32): 5}
        arrs = [np.ascontiguousarray(a) for a in (xyz, time, laser_id, intensity)]
        mp = np.ascontiguousarray(mapping, np.uint16) if mapping is not None else None
        stamp, kept = C.c_uint64(0), C.c_int(0)
        f = self.L.lsa_upload_polydata_frame
        f.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p, C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
        args = []
        for a in arrs:
            args += [a.ctypes.data_as(C.c_void_p), codes[a.dtype]]
        rc = self._check(f(self.h, arrs[1].size, *args, ptr(mp) if mp is not None else None, 0 if mp is None else mp.size, C.c_double(time_to_seconds),
                           C.byref(stamp), C.byref(kept)), "lsa_upload_polydata_frame")
        return stamp.value, kept.value, rc == 1

    def extract_keypoints(self, params=None):
        params = params or ExtractParams()
        counts = np.zeros(3, np.int32)
        self._check(self.L.lsa_extract_keypoints(self.h, C.byref(params), ptr(counts)), "lsa_extract_keypoints")
        return counts

    def keypoints(self, kset, ktype):
        n = self.L.lsa_keypoint_count(self.h, kset, ktype)
        out = np.zeros(max(n, 0), POINT_DTYPE)
        if n > 0:
            self._check(self.L.lsa_download_keypoints(self.h, kset, ktype, ptr(out), n), "lsa_download_keypoints")
        return out

    def set_keypoints(self, kset, ktype, pts):
        pts = np.ascontiguousarray(pts)
        self._check(self.L.lsa_set_keypoints(self.h, kset, ktype, ptr(pts) if pts.size else None, pts.size), "lsa_set_keypoints")

    def debug_array(self, array_id):
        n = self.L.lsa_frame_size(self.h)
        out = np.zeros(n, np.float32)
        self._check(self.L.lsa_download_debug(self.h, array_id, ptr(out), n), "lsa_download_debug")
        return out

    def nb_laser_rings(self):
        return self.L.lsa_nb_laser_rings(self.h)

    def transform_keypoints(self, kset, ktype, T, time_offset=0.0):
        self._check(self.L.lsa_transform_keypoints(self.h, kset, ktype, ptr(pose16(T)), time_offset), "lsa_transform_keypoints")

    # ---- matching
    def set_target(self, ktype, pts, cell=None, slot=TARGET_MAP):
        pts = np.ascontiguousarray(pts)
        if cell is not None:
            self.L.lsa_set_target_cell_size(self.h, slot, ktype, cell)
        self._check(self.L.lsa_set_target(self.h, slot, ktype, ptr(pts) if pts.size else None, pts.size), "lsa_set_target")

    def set_target_from_set(self, ktype, kset, cell=None, slot=TARGET_PREVIOUS):
        if cell is not None:
            self.L.lsa_set_target_cell_size(self.h, slot, ktype, cell)
        self._check(self.L.lsa_set_target_from_set(self.h, slot, ktype, kset), "lsa_set_target_from_set")

    def stage_target(self, ktype, pts, ahead=False, cell=None, slot=TARGET_MAP):
        """lsa_target_staging + lsa_stage_target_ahead / lsa_set_target_staged: the points are written into the
        target's pinned staging buffer, then either handed to the device ahead of time (ahead=True) or made the target"""
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        self.L.lsa_target_staging.restype = C.c_void_p
        self.L.lsa_target_staging.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        buf = self.L.lsa_target_staging(self.h, slot, ktype, pts.size)
        if not buf and pts.size:
            raise LsaError("lsa_target_staging failed")
        if pts.size:
            C.memmove(buf, pts.ctypes.data, pts.nbytes)
        if cell is not None:
            self.L.lsa_set_target_cell_size(self.h, slot, ktype, cell)
        if ahead:
            self._check(self.L.lsa_stage_target_ahead(self.h, slot, ktype, pts.size), "lsa_stage_target_ahead")
        else:
            self._check(self.L.lsa_set_target_staged(self.h, slot, ktype, pts.size), "lsa_set_target_staged")

    def drop_target_ahead(self, ktype, slot=TARGET_MAP):
        self._check(self.L.lsa_drop_target_ahead(self.h, slot, ktype), "lsa_drop_target_ahead")

    def prepare_previous_targets(self, type_mask):
        self._check(self.L.lsa_prepare_previous_targets(self.h, type_mask), "lsa_prepare_previous_targets")

    def target(self, ktype, slot=TARGET_MAP):
        n = self.L.lsa_target_size(self.h, slot, ktype)
        out = np.zeros(max(n, 0), POINT_DTYPE)
        if n > 0:
            self._check(self.L.lsa_download_target(self.h, slot, ktype, ptr(out), n), "lsa_download_target")
        return out

    def match(self, ktype, query_set, params, pose, slot=TARGET_MAP):
        hist = np.zeros(MATCH_NSTATUS, np.int32)
        self._check(self.L.lsa_match(self.h, slot, ktype, query_set, C.byref(params), ptr(pose16(pose)), ptr(hist)), "lsa_match")
        return hist

    def match_types(self, type_mask, query_set, params, pose, slot=TARGET_MAP, histograms=True):
        """lsa_match_types: the types in type_mask matched concurrently; returns [3][NSTATUS] or None (async)."""
        hist = np.zeros((3, 8), np.int32) if histograms else None
        self._check(self.L.lsa_match_types(self.h, slot, type_mask, query_set, C.byref(params), ptr(pose16(pose)),
                                           ptr(hist) if histograms else None), "lsa_match_types")
        return hist

    def match_types_undistorted(self, type_mask, params, pose, H0, H1, t0, t1, slot=TARGET_MAP):
        """lsa_match_types_undistorted: lsa_undistort + lsa_match_types on the working set, the undistortion inside the search
        kernel where it can be; returns [3][NSTATUS]"""
        hist = np.zeros((3, 8), np.int32)
        self._check(self.L.lsa_match_types_undistorted(self.h, slot, type_mask, C.byref(params), ptr(pose16(pose)), ptr(hist), ptr(pose16(H0)), ptr(pose16(H1)),
                                                       C.c_double(t0), C.c_double(t1)), "lsa_match_types_undistorted")
        return hist

    def overlap(self, type_mask, ratio, leaves, H0, H1=None, t0=0.0, t1=0.0):
        """lsa_overlap: LCP overlap estimate of the current frame against the map-slot targets."""
        out = C.c_float(-1.0)
        lf = (C.c_double * 3)(*[float(x) for x in leaves])
        self._check(self.L.lsa_overlap(self.h, type_mask, int(H1 is not None), ptr(pose16(H0)), ptr(pose16(H1)) if H1 is not None else None,
                                       C.c_double(t0), C.c_double(t1), C.c_float(ratio), lf, C.byref(out)), "lsa_overlap")
        return float(out.value)

    def upload_match(self, ktype, status, records, saturation):
        """lsa_upload_match (test hook): the match buffer of `ktype` becomes these rows (n, 16), their status and the saturation distance"""
        status = np.ascontiguousarray(status, np.uint8)
        records = np.ascontiguousarray(records, np.float64).reshape(-1, 16)
        assert records.shape[0] == status.size
        self._check(self.L.lsa_upload_match(self.h, ktype, ptr(status), ptr(records), status.size, C.c_double(saturation)), "lsa_upload_match")

    def knn_lists(self, ktype, capacity):
        """lsa_download_knn (test hook): (idx (n, 16) int32, d2 (n, 16) float32, cnt (n,) int32) of the first
        min(capacity, queries) queries of the last search of `ktype` that left its neighbour lists in memory; cnt -1: k-th neighbour beyond the rejection distance, -2: whole-target search"""
        idx = np.zeros((capacity, KNN_MAX), np.int32)
        d2 = np.zeros((capacity, KNN_MAX), np.float32)
        cnt = np.zeros(capacity, np.int32)
        n = self._check(self.L.lsa_download_knn(self.h, ktype, ptr(idx), ptr(d2), ptr(cnt), capacity), "lsa_download_knn")
        return idx[:n], d2[:n], cnt[:n]

    def match_results(self, ktype, query_set=None, records=True, n=None):
        if n is None:
            n = self.L.lsa_keypoint_count(self.h, SET_WORKING if query_set is None else query_set, ktype)
        n = max(n, 0)
        status = np.zeros(n, np.uint8)
        weights = np.zeros(n, np.float64)
        rec = np.zeros((n, 16), np.float64) if records else None
        got = self._check(
            self.L.lsa_download_match(self.h, ktype, ptr(status), ptr(weights), ptr(rec) if records else None, n), "lsa_download_match"
        )
        return status[:got], weights[:got], (rec[:got] if records else None)

    def route_stats(self, ktype):
        out = np.zeros(8, np.int32)
        self.L.lsa_match_route_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self._check(self.L.lsa_match_route_stats(self.h, ktype, ptr(out)), "lsa_match_route_stats")
        return out

    def match_trace(self, blocks):
        out = np.zeros((blocks, 12), np.uint64)
        self.L.lsa_match_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self._check(self.L.lsa_match_trace(self.h, ptr(out), blocks), "lsa_match_trace")
        return out

    def set_fused_match(self, on):
        self._check(self.L.lsa_set_fused_match(self.h, int(on)), "lsa_set_fused_match")

    def slow_queries(self):
        return self.L.lsa_match_slow_queries(self.h)

    def accumulate(self, type_mask, w, jac=True):
        w = np.ascontiguousarray(w, np.float64)
        cost = C.c_double()
        nv = C.c_int()
        g = np.zeros(6)
        H = np.zeros((6, 6))
        self._check(self.L.lsa_accumulate(self.h, type_mask, ptr(w), int(jac), C.byref(cost), ptr(g), ptr(H), C.byref(nv)), "lsa_accumulate")
        return cost.value, g, H, nv.value

    def solve(self, type_mask, prior, max_iter=15, two_d=False):
        """LocalOptimizer::Solve on the device residuals: (pose 4x4, summary[4], costs[2])."""
        out = np.zeros(16)
        summ = np.zeros(4, np.int32)
        costs = np.zeros(2)
        self._check(self.L.lsa_solve(self.h, type_mask, ptr(pose16(prior)), max_iter, int(two_d), ptr(out), ptr(summ), ptr(costs)), "lsa_solve")
        return out.reshape(4, 4), summ, costs

    def solve_device(self, type_mask, prior6, max_iter=15, two_d=False, min_matches=0):
        """LocalOptimizer::Solve as one launch (the trust-region loop runs on the device): SolveResult."""
        r = SolveResult()
        w = np.ascontiguousarray(prior6, np.float64)
        self._check(self.L.lsa_solve_device(self.h, type_mask, ptr(w), int(two_d), max_iter, min_matches, C.byref(r)), "lsa_solve_device")
        return r

    def solve_device_begin(self, type_mask, prior6=None, max_iter=15, two_d=False, min_matches=0):
        """lsa_solve_device_begin; prior6 None: the start point comes from the link the solve before it leaves (icp_link)"""
        w = None if prior6 is None else np.ascontiguousarray(prior6, np.float64)
        self.L.lsa_solve_device_begin.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_int, C.c_int, C.c_int]
        self._check(self.L.lsa_solve_device_begin(self.h, type_mask, None if w is None else ptr(w), int(two_d), max_iter, min_matches), "lsa_solve_device_begin")

    def solve_device_end(self):
        """lsa_solve_device_end -> SolveResult, or the negative code (LSA_E_STATE ...) when there is none"""
        r = SolveResult()
        self.L.lsa_solve_device_end.argtypes = [C.c_void_p, C.c_void_p]
        rc = self.L.lsa_solve_device_end(self.h, C.byref(r))
        return r if rc == 0 else rc

    def solve_device_drop(self):
        self.L.lsa_solve_device_drop.argtypes = [C.c_void_p]
        self._check(self.L.lsa_solve_device_drop(self.h), "lsa_solve_device_drop")

    def icp_link(self):
        """lsa_icp_link: reserves the block the next linked solve leaves for the iteration behind it -> ticket"""
        self.L.lsa_icp_link.argtypes = [C.c_void_p]
        return self._check(self.L.lsa_icp_link(self.h), "lsa_icp_link")

    def solve_device_begin_linked(self, type_mask, prior6, leave_ticket, link, max_iter=15, two_d=False, min_matches=0):
        w = None if prior6 is None else np.ascontiguousarray(prior6, np.float64)
        self.L.lsa_solve_device_begin_linked.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        self._check(self.L.lsa_solve_device_begin_linked(self.h, type_mask, None if w is None else ptr(w), int(two_d), max_iter, min_matches, leave_ticket,
                                                         None if link is None else C.byref(link)), "lsa_solve_device_begin_linked")

    def icp_link_peek(self, ticket):
        out = np.zeros(64, np.uint64)
        self.L.lsa_icp_link_peek.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        self._check(self.L.lsa_icp_link_peek(self.h, ticket, ptr(out)), "lsa_icp_link_peek")
        return out

    def icp_cancel(self, ticket):
        self.L.lsa_icp_cancel.argtypes = [C.c_void_p, C.c_int]
        self._check(self.L.lsa_icp_cancel(self.h, ticket), "lsa_icp_cancel")

    def icp_abandon(self):
        self.L.lsa_icp_abandon.argtypes = [C.c_void_p]
        self._check(self.L.lsa_icp_abandon(self.h), "lsa_icp_abandon")

    def match_types_linked(self, type_mask, query_set, params, undistort=False, slot=TARGET_MAP):
        """lsa_match_types_linked: 0 enqueued behind the link reserved last, 1 this match cannot wait behind a link"""
        self.L.lsa_match_types_linked.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_int, C.c_void_p, C.c_int]
        return self._check(self.L.lsa_match_types_linked(self.h, slot, type_mask, query_set, C.byref(params), int(undistort)), "lsa_match_types_linked")

    def profile_event_overhead_us(self):
        self.L.lsa_profile_event_overhead_us.restype = C.c_double
        self.L.lsa_profile_event_overhead_us.argtypes = [C.c_void_p]
        return float(self.L.lsa_profile_event_overhead_us(self.h))

    def debug_set(self, name, value):
        self.L.lsa_debug_set.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        self._check(self.L.lsa_debug_set(self.h, name.encode(), int(value)), "lsa_debug_set")

    def solve_device_trace(self):
        out = np.zeros(12, np.uint64)
        self.L.lsa_solve_device_trace.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.L.lsa_solve_device_trace(self.h, ptr(out)), "lsa_solve_device_trace")
        return out

    def solve_device_fallbacks(self):
        return self.L.lsa_solve_device_fallbacks(self.h)

    def solve_device_shape(self):
        """(workgroups, residual blocks per thread, of those in LDS, total) of the last one-launch solve"""
        out = np.zeros(4, np.int32)
        self._check(self.L.lsa_solve_device_shape(self.h, ptr(out)), "lsa_solve_device_shape")
        return tuple(int(v) for v in out)

    def accumulate_shape(self):
        """(workgroups, most residual blocks of a thread, 0, total) of the last accumulate"""
        out = np.zeros(4, np.int32)
        self._check(self.L.lsa_accumulate_shape(self.h, ptr(out)), "lsa_accumulate_shape")
        return tuple(int(v) for v in out)

    def set_sensor_terms(self, terms=None):
        """lsa_set_sensor_terms: a SensorTerms enters every accumulate / solve / registration error from now on; None clears"""
        self._check(self.L.lsa_set_sensor_terms(self.h, C.byref(terms) if terms is not None else None), "lsa_set_sensor_terms")

    def registration_error(self, type_mask, pose, two_d=False):
        cov = np.zeros((6, 6))
        err = np.zeros(2)
        self._check(self.L.lsa_registration_error(self.h, type_mask, ptr(pose16(pose)), int(two_d), ptr(cov), ptr(err)), "lsa_registration_error")
        return cov, err

    def selftest_math(self, fn, x, y=None):
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(x if y is None else y, np.float64)
        out = np.zeros_like(x)
        self._check(self.L.lsa_selftest_math(self.h, fn, ptr(x), ptr(y), x.size, ptr(out)), "lsa_selftest_math")
        return out

    def selftest_numerics(self, fn, records):
        """lsa_selftest_numerics on the device (fn 0-7) or the host twins (fn 8-11): records (n, IN) -> (n, OUT)"""
        return selftest_numerics(fn, records, self)

    def selftest_labels(self, ring_lengths, sin_angle, depth_gap, saliency, intensity_gap, valid, params=None):
        """lsa_selftest_labels: the labelling kernel alone on the given scores and validity bytes, rings one after the
        other -> (label, validity afterwards, ring_counts (nrings, 3))"""
        params = params or ExtractParams()
        lens = np.ascontiguousarray(ring_lengths, np.int32)
        n = int(lens.sum())
        scores = [np.ascontiguousarray(a, np.float32) for a in (sin_angle, depth_gap, saliency, intensity_gap)]
        valid = np.ascontiguousarray(valid, np.uint8)
        assert all(a.size == n for a in scores) and valid.size == n
        label, after, counts = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((lens.size, 3), np.int32)
        self._check(self.L.lsa_selftest_labels(self.h, C.byref(params), ptr(lens), lens.size, *[ptr(a) for a in scores], ptr(valid), ptr(label),
                                               ptr(after), ptr(counts)), "lsa_selftest_labels")
        return label, after, counts

    # ---- undistortion / transforms
    def reset_working_keypoints(self):
        self._check(self.L.lsa_reset_working_keypoints(self.h), "lsa_reset_working_keypoints")

    def undistort(self, H0, H1, t0, t1):
        self._check(self.L.lsa_undistort(self.h, ptr(pose16(H0)), ptr(pose16(H1)), t0, t1), "lsa_undistort")

    def localization_begin(self, H0=None, H1=None, t0=0.0, t1=0.0, box_pose=None, arm=False):
        """lsa_localization_begin: reset + undistort (unless H0 is None) + boxes under box_pose (unless None), one launch;
        the boxes are read with keypoint_bboxes_end"""
        if arm:
            self._check(self.L.lsa_arm_localization_boxes(self.h), "lsa_arm_localization_boxes")
        self._check(self.L.lsa_localization_begin(self.h, ptr(pose16(H0)) if H0 is not None else None, ptr(pose16(H1)) if H1 is not None else None,
                                                  C.c_double(t0), C.c_double(t1), ptr(pose16(box_pose)) if box_pose is not None else None), "lsa_localization_begin")

    def keypoint_bboxes_end(self):
        mn, mx = np.zeros(9, np.float32), np.zeros(9, np.float32)
        self._check(self.L.lsa_keypoint_bboxes_end(self.h, ptr(mn), ptr(mx)), "lsa_keypoint_bboxes_end")
        return mn.reshape(3, 3), mx.reshape(3, 3)

    def working_time_range(self):
        a, b = C.c_double(), C.c_double()
        self._check(self.L.lsa_working_time_range(self.h, C.byref(a), C.byref(b)), "lsa_working_time_range")
        return a.value, b.value

    def keypoint_time_range(self, kset):
        a, b = C.c_double(), C.c_double()
        self._check(self.L.lsa_keypoint_time_range(self.h, kset, C.byref(a), C.byref(b)), "lsa_keypoint_time_range")
        return a.value, b.value

    def keypoint_bboxes(self, kset, H0, H1=None, t0=0.0, t1=0.0):
        """bounding boxes of the three keypoint types of a set under a pose, or under the pose interpolated at
        every point's time between H0 (t0) and H1 (t1); returns (mn[3][3], mx[3][3])"""
        if H1 is None:
            self._check(self.L.lsa_keypoint_bboxes_begin(self.h, kset, ptr(pose16(H0))), "lsa_keypoint_bboxes_begin")
        else:
            self._check(self.L.lsa_keypoint_bboxes_begin_interp(self.h, kset, ptr(pose16(H0)), ptr(pose16(H1)), C.c_double(t0), C.c_double(t1)),
                        "lsa_keypoint_bboxes_begin_interp")
        mn, mx = np.zeros(9, np.float32), np.zeros(9, np.float32)
        self._check(self.L.lsa_keypoint_bboxes_end(self.h, ptr(mn), ptr(mx)), "lsa_keypoint_bboxes_end")
        return mn.reshape(3, 3), mx.reshape(3, 3)

    def match_serial(self, ktype):
        return self.L.lsa_match_serial(self.h, ktype)

    def match_histogram(self, ktype, serial):
        h = np.zeros(8, np.int32)
        self._check(self.L.lsa_match_histogram(self.h, ktype, serial, ptr(h)), "lsa_match_histogram")
        return h

    def working_bbox(self, ktype, pose):
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._check(self.L.lsa_working_bbox(self.h, ktype, ptr(pose16(pose)), ptr(mn), ptr(mx)), "lsa_working_bbox")
        return mn, mx

    def transformed_keypoints(self, kset, ktype, pose):
        n = max(self.L.lsa_keypoint_count(self.h, kset, ktype), 0)
        out = np.zeros(n, POINT_DTYPE)
        if n:
            self._check(self.L.lsa_download_transformed(self.h, kset, ktype, ptr(pose16(pose)), ptr(out), n), "lsa_download_transformed")
        return out

    def transform_frame(self, H0, H1=None, t0=0.0, t1=0.0):
        n = self.L.lsa_frame_size(self.h)
        out = np.zeros(n, POINT_DTYPE)
        interp = H1 is not None
        self._check(
            self.L.lsa_transform_frame(self.h, int(interp), ptr(pose16(H0)), ptr(pose16(H1)) if interp else None, t0, t1, ptr(out), n),
            "lsa_transform_frame",
        )
        return out

    # ---- profiling
    def profile(self, on=True):
        self.L.lsa_profile_enable(self.h, int(on))

    def profile_select(self, scope, every=1):
        self.L.lsa_profile_select(self.h, scope.encode(), int(every))

    def profile_reset(self):
        self.L.lsa_profile_reset(self.h)

    def profile_stats(self):
        return _profile(self.L, self.h)

    def sync(self):
        self._check(self.L.lsa_sync(self.h), "lsa_sync")

    # ---- the keypoint log (lsa_kplog_*): frames of raw keypoints in device memory, replayed under a trajectory
    def kplog_append(self):
        """a frame from the SET_RAW_CURRENT keypoints"""
        self._check(self.L.lsa_kplog_append(self.h), "lsa_kplog_append")

    def kplog_append_points(self, frame):
        """a frame of the caller's keypoints: three arrays (edges, planes, blobs), any of them empty"""
        arrs = [np.ascontiguousarray(a, POINT_DTYPE) for a in frame]
        ptrs = (C.c_void_p * 3)(*[a.ctypes.data if a.size else None for a in arrs])
        ns = (C.c_int * 3)(*[a.size for a in arrs])
        self._check(self.L.lsa_kplog_append_points(self.h, ptrs, ns), "lsa_kplog_append_points")

    def kplog_pop_front(self):
        self._check(self.L.lsa_kplog_pop_front(self.h), "lsa_kplog_pop_front")

    def kplog_clear(self):
        self._check(self.L.lsa_kplog_clear(self.h), "lsa_kplog_clear")

    def kplog_size(self):
        return self.L.lsa_kplog_size(self.h)

    def kplog_count(self, frame, ktype):
        return self._check(self.L.lsa_kplog_count(self.h, frame, ktype), "lsa_kplog_count")

    def kplog_get(self, frame, ktype):
        out = np.zeros(max(self.kplog_count(frame, ktype), 1), POINT_DTYPE)
        n = self._check(self.L.lsa_kplog_get(self.h, frame, ktype, ptr(out), out.size), "lsa_kplog_get")
        return out[:n].copy()

    def kplog_bytes(self):
        return int(self.L.lsa_kplog_bytes(self.h))

    def kplog_stopped(self):
        return bool(self.L.lsa_kplog_stopped(self.h))

    def kplog_replay(self, poses, times, undistort=True, type_mask=7):
        """every logged frame under poses (n, 4, 4) dated times (n,) -> ([edges, planes, blobs] frames ascending,
        last frame's min [3][3], max [3][3])"""
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        t = np.ascontiguousarray(times, np.float64)
        n = self.kplog_size()
        outs = [np.zeros(max(sum(self.kplog_count(f, k) for f in range(n)) if (type_mask >> k) & 1 else 0, 1), POINT_DTYPE) for k in range(3)]
        ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
        mn, mx = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
        self._check(self.L.lsa_kplog_replay(self.h, type_mask, ptr(P), ptr(t), P.shape[0], int(bool(undistort)), ptrs, ptr(mn), ptr(mx)), "lsa_kplog_replay")
        sizes = [int(self.L.lsa_kplog_replayed(self.h, k, C.byref(C.c_void_p()))) for k in range(3)]
        return [o[:s].copy() for o, s in zip(outs, sizes)], mn, mx

    def kplog_replay_range(self, poses, times, first, last, rule, type_mask=7):
        """the logged frames first..last (inclusive) under poses (n, 4, 4) dated times (n,) of ALL logged frames; rule 0 rigid,
        1 the rebuild's times (t[i] - t[i-1], 0), 2 the sweep's (-(t[i] - t[i-1]), 0) -> ([edges, planes, blobs] frames
        ascending, min [3][3], max [3][3] of all replayed points per type)"""
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        t = np.ascontiguousarray(times, np.float64)
        frames = range(max(first, 0), min(last, self.kplog_size() - 1) + 1)
        outs = [np.zeros(max(sum(self.kplog_count(f, k) for f in frames) if (type_mask >> k) & 1 else 0, 1), POINT_DTYPE) for k in range(3)]
        ptrs = (C.c_void_p * 3)(*[o.ctypes.data for o in outs])
        mn, mx = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
        self._check(self.L.lsa_kplog_replay_range(self.h, type_mask, ptr(P), ptr(t), P.shape[0], int(first), int(last), int(rule), ptrs, ptr(mn), ptr(mx)),
                    "lsa_kplog_replay_range")
        sizes = [int(self.L.lsa_kplog_replayed(self.h, k, C.byref(C.c_void_p()))) for k in range(3)]
        return [o[:s].copy() for o, s in zip(outs, sizes)], mn, mx

    # ---- the log's descriptor store (lsa_kplog_describe / _descriptors / _place_search): place recognition
    # ---- pose graph (lsa_pose_graph.hip); the module functions of the same names without a Context are the host statement
    def pose_graph_solve(self, poses, fixed, edges, params=None, priors=None, offset=None, **kw):
        return pose_graph_solve(poses, fixed, edges, self, params, priors, offset, **kw)

    def pose_graph_linearize_priors(self, poses, priors, offset=None):
        return pose_graph_linearize_priors(poses, priors, offset, self)

    def pose_graph_premultiply(self, poses, W):
        return pose_graph_premultiply(poses, W, self)

    def pose_graph_reanchor(self, poses):
        return pose_graph_reanchor(poses, self)

    def pose_graph_linearize(self, poses, edges):
        return pose_graph_linearize(poses, edges, self)

    def pose_graph_assemble(self, poses, fixed, edges, lam=0.0, priors=None, offset=None):
        return pose_graph_assemble(poses, fixed, edges, lam, self, priors, offset)

    def pose_graph_spmv(self, poses, fixed, edges, lam, p, priors=None, offset=None):
        return pose_graph_spmv(poses, fixed, edges, lam, p, self, priors, offset)

    def pose_graph_tridiagonal_solve(self, D, L, U, b):
        return pose_graph_tridiagonal_solve(D, L, U, b, self)

    def pose_graph_retract(self, poses, delta):
        return pose_graph_retract(poses, delta, self)

    def kplog_describe(self, first, last, **params):
        """describes the frames first..last that have no valid descriptor under these PlaceParams -> how many it described"""
        p = PlaceParams(**params)
        return self._check(self.L.lsa_kplog_describe(self.h, C.byref(p), int(first), int(last)), "lsa_kplog_describe")

    def kplog_descriptors(self, first, last, **params):
        """the described frames' descriptors -> float32 (last - first + 1, PlaceParams(**params).length)"""
        length = PlaceParams(**params).length
        if self.L.lsa_kplog_descriptor_length(self.h) not in (0, length):
            raise _error("lsa_kplog_descriptors", E_STATE, "the store holds descriptors of another shape")
        out = np.zeros((max(int(last) - int(first) + 1, 1), max(length, 1)), np.float32)
        self._check(self.L.lsa_kplog_descriptors(self.h, int(first), int(last), ptr(out)), "lsa_kplog_descriptors")
        return out

    def kplog_place_search(self, query, first, last, out=None, **params):
        """frame `query` against the frames first..last -> (distance float32 (count,), shift int32 (count,)), written into
        out = (distance, shift) where given"""
        p = PlaceParams(**params)
        count = max(int(last) - int(first) + 1, 1)
        d, s = out if out is not None else (np.zeros(count, np.float32), np.zeros(count, np.int32))
        self._check(self.L.lsa_kplog_place_search(self.h, C.byref(p), int(query), int(first), int(last), ptr(d), ptr(s)), "lsa_kplog_place_search")
        return d, s

    def kplog_described(self):
        """frames described by the last kplog_describe / kplog_place_search"""
        return self.L.lsa_kplog_described(self.h)

    def kplog_replay_to_grids(self, poses, times, grids, undistort=True):
        """the same straight into device maps of this context: grids = [edges, planes, blobs], a DeviceGrid or None each;
        per map ONE Add(aggregate, fixed=False, time=-1, roll=False), nothing comes to the host.  Returns the last
        frame's min [3][3], max [3][3] (what the caller rolls the maps onto)."""
        P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
        t = np.ascontiguousarray(times, np.float64)
        mask = sum(1 << k for k in range(3) if grids[k] is not None)
        hs = (C.c_void_p * 3)(*[g.h.value if g is not None else None for g in grids])
        mn, mx = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
        self._check(self.L.lsa_kplog_replay_to_grids(self.h, mask, ptr(P), ptr(t), P.shape[0], int(bool(undistort)), hs, ptr(mn), ptr(mx)), "lsa_kplog_replay_to_grids")
        return mn, mx


class Slam:
    """LidarSlam::Slam on one MI355X.  Parameters use the reference's names (``EgoMotion=3`` ...)."""

    def __init__(self, device=0, **params):
        self.L = lib()
        h = C.c_void_p()
        rc = self.L.lsa_slam_create(device, C.byref(h))
        if rc != 0:
            raise LsaError(f"lsa_slam_create({device}) failed with {rc}: no usable HIP device (there is no CPU fallback)")
        self.h = h
        self._n = 0
        for k, v in params.items():
            self.set_param(k, v)

    def close(self):
        if getattr(self, "h", None):
            self.L.lsa_slam_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise _error(what, rc, self.L.lsa_slam_last_error(self.h).decode())
        return rc

    def set_param(self, name, value):
        if self.L.lsa_slam_set_param(self.h, name.encode(), float(value)) != 0:
            raise KeyError(name)

    def get_param(self, name):
        v = C.c_double()
        if self.L.lsa_slam_get_param(self.h, name.encode(), C.byref(v)) != 0:
            raise KeyError(name)
        return v.value

    def reset(self, reset_log=True):
        self.L.lsa_slam_reset(self.h, int(reset_log))

    # external sensors (Slam::AddWheelOdomMeasurement / AddGravityMeasurement / ClearSensorMeasurements); the weights and
    # the time offset are the parameters WheelOdomWeight, GravityWeight and SensorTimeOffset
    def add_wheel_odom(self, time, distance):
        self._check(self.L.lsa_slam_add_wheel_odom_measurement(self.h, float(time), float(distance)), "lsa_slam_add_wheel_odom_measurement")

    def add_gravity(self, time, acc):
        a = np.ascontiguousarray(acc, np.float64)
        self._check(self.L.lsa_slam_add_gravity_measurement(self.h, float(time), ptr(a)), "lsa_slam_add_gravity_measurement")

    def clear_sensor_measurements(self):
        self._check(self.L.lsa_slam_clear_sensor_measurements(self.h), "lsa_slam_clear_sensor_measurements")

    def sensor_terms(self):
        """the SensorTerms the last frame's localization solved with"""
        t = SensorTerms()
        self._check(self.L.lsa_slam_sensor_terms(self.h, C.byref(t)), "lsa_slam_sensor_terms")
        return t

    def add_frame(self, pts, stamp_us, seq=0):
        """Slam::AddFrame: host scan -> pose."""
        pts = np.ascontiguousarray(pts)
        assert pts.dtype == POINT_DTYPE
        self._n = pts.size
        self._check(self.L.lsa_slam_add_frame(self.h, ptr(pts), pts.size, stamp_us, seq), "lsa_slam_add_frame")

    def store_frame(self, slot, pts):
        pts = np.ascontiguousarray(pts)
        self._check(self.L.lsa_slam_store_frame(self.h, slot, ptr(pts), pts.size), "lsa_slam_store_frame")

    def hint_next_stored_frame(self, slot):
        """replay: the slot that will be added after the next add_stored_frame (its extraction is overlapped)"""
        self._check(self.L.lsa_slam_hint_next_stored_frame(self.h, slot), "lsa_slam_hint_next_stored_frame")

    def hint_next_frame(self, pts):
        """replay from host clouds: the array of the add_frame call after the next one; its upload and extraction overlap
        the frame in between.  The very same (contiguous) array must then be passed to add_frame and stay alive until then."""
        self._check(self.L.lsa_slam_hint_next_frame(self.h, ptr(pts), pts.size), "lsa_slam_hint_next_frame")

    def add_stored_frame(self, slot, stamp_us, seq=0):
        self._check(self.L.lsa_slam_add_stored_frame(self.h, slot, stamp_us, seq), "lsa_slam_add_stored_frame")

    # replay loops that hold their clouds for the whole run: the pointer of a cloud is taken once (`cloud_pointer`), not per call
    @staticmethod
    def pin_cloud(pts):
        """lsa_pin_host_memory on the array's buffer (a driver's scan buffer that is handed over again and again)"""
        L = lib()
        L.lsa_pin_host_memory.argtypes = [C.c_void_p, C.c_size_t]
        if L.lsa_pin_host_memory(ptr(pts), pts.nbytes) != 0:
            raise LsaError("lsa_pin_host_memory failed")

    @staticmethod
    def unpin_cloud(pts):
        L = lib()
        L.lsa_unpin_host_memory.argtypes = [C.c_void_p]
        L.lsa_unpin_host_memory(ptr(pts))

    @staticmethod
    def cloud_pointer(pts):
        assert pts.dtype == POINT_DTYPE
        return ptr(pts), int(pts.size)

    def add_frame_at(self, cloud, stamp_us, seq=0):
        """add_frame on a (pointer, size) pair from `cloud_pointer`; the array it came from must be alive"""
        self._n = cloud[1]
        self._check(self.L.lsa_slam_add_frame(self.h, cloud[0], cloud[1], stamp_us, seq), "lsa_slam_add_frame")

    def hint_next_frame_at(self, cloud):
        self._check(self.L.lsa_slam_hint_next_frame(self.h, cloud[0], cloud[1]), "lsa_slam_hint_next_frame")

    def stats_into(self, out_ptr):
        """stats() into an array the caller keeps (out_ptr = ptr(np.zeros(16)))"""
        self.L.lsa_slam_get_stats(self.h, out_ptr)

    def world_transform(self):
        T = np.zeros(16)
        t = C.c_double()
        self.L.lsa_slam_get_world_transform(self.h, ptr(T), C.byref(t))
        return T.reshape(4, 4)

    def covariance(self):
        c = np.zeros((6, 6))
        self.L.lsa_slam_get_covariance(self.h, ptr(c))
        return c

    def latency_compensated_world_transform(self):
        T = np.zeros(16)
        t = C.c_double()
        self._check(self.L.lsa_slam_get_latency_compensated_world_transform(self.h, ptr(T), C.byref(t)), "latency compensated transform")
        return T.reshape(4, 4)

    def set_world_transform_from_guess(self, T):
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        self._check(self.L.lsa_slam_set_world_transform_from_guess(self.h, ptr(T)), "lsa_slam_set_world_transform_from_guess")

    def add_frames(self, frames, stamps_us, seq=0):
        """Slam::AddFrames: one frame per LiDAR device, each with its own stamp"""
        frames = [np.ascontiguousarray(f, POINT_DTYPE) for f in frames]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data if f.size else None for f in frames])
        sizes = np.array([f.size for f in frames], np.int32)
        stamps = np.array(stamps_us, np.uint64)
        seqs = np.full(len(frames), seq, np.uint32)
        self._n = max(self._n, int(sizes.sum()))
        return self._check(self.L.lsa_slam_add_frames(self.h, ptrs, ptr(sizes), ptr(stamps), ptr(seqs), len(frames)), "lsa_slam_add_frames")

    def set_extractor_param(self, device_id, name, value):
        self._check(self.L.lsa_slam_set_extractor_param(self.h, device_id, name.encode(), float(value)), "lsa_slam_set_extractor_param")

    def extractor_param(self, device_id, name):
        v = C.c_double()
        self._check(self.L.lsa_slam_get_extractor_param(self.h, device_id, name.encode(), C.byref(v)), "lsa_slam_get_extractor_param")
        return v.value

    def set_base_to_lidar_offset(self, T, device_id=0):
        T = np.ascontiguousarray(T, np.float64).reshape(16)
        self._check(self.L.lsa_slam_set_base_to_lidar_offset(self.h, ptr(T), device_id), "lsa_slam_set_base_to_lidar_offset")

    def base_to_lidar_offset(self, device_id=0):
        T = np.zeros(16)
        self._check(self.L.lsa_slam_get_base_to_lidar_offset(self.h, ptr(T), device_id), "lsa_slam_get_base_to_lidar_offset")
        return T.reshape(4, 4)

    def trajectory(self):
        """Slam::GetTrajectory / GetCovariances: (n, 4, 4) poses, (n,) times [s], (n, 6, 6) covariances"""
        n = self._check(self.L.lsa_slam_get_trajectory(self.h, None, None, 0), "lsa_slam_get_trajectory")
        rows, cov = np.zeros((max(n, 1), 17)), np.zeros((max(n, 1), 36))
        self.L.lsa_slam_get_trajectory(self.h, ptr(rows), ptr(cov), n)
        return rows[:n, :16].reshape(n, 4, 4).copy(), rows[:n, 16].copy(), cov[:n].reshape(n, 6, 6).copy()

    def debug_information(self):
        """Slam::GetDebugInformation with the reference's keys (+ "latency")"""
        o = np.zeros(10)
        self._check(self.L.lsa_slam_get_debug_information(self.h, ptr(o)), "lsa_slam_get_debug_information")
        return dict(zip(DEBUG_INFORMATION_NAMES, o.tolist()))

    def map(self, ktype, clean=False):
        """Slam::GetMap(k, clean)"""
        n = self._check(self.L.lsa_slam_get_map(self.h, ktype, int(clean), None, 0), "lsa_slam_get_map")
        out = np.zeros(max(n, 1), POINT_DTYPE)
        n = self.L.lsa_slam_get_map(self.h, ktype, int(clean), ptr(out), out.size)
        return out[:n].copy()

    def add_map_points(self, ktype, pts, fixed=False, time=-1.0):
        """RollingGrid::Add(pts, fixed, time) on the map of one keypoint type"""
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        self._check(self.L.lsa_slam_add_map_points(self.h, ktype, ptr(pts) if pts.size else None, pts.size, int(fixed), float(time)), "lsa_slam_add_map_points")

    def map_io_counts(self):
        o = np.zeros(3, np.int32)
        self.L.lsa_slam_map_io_counts(self.h, ptr(o))
        return o.tolist()

    def save_maps_pcd(self, prefix, fmt=PCD_BINARY, filtered=True):
        """Slam::SaveMapsToPCD: <prefix>edges.pcd ...; returns the points written per type (-1: no file)"""
        self._check(self.L.lsa_slam_save_maps_pcd(self.h, os.fsencode(prefix), int(fmt), int(filtered)), "lsa_slam_save_maps_pcd")
        return self.map_io_counts()

    def load_maps_pcd(self, prefix, reset_maps=True, time=-1.0):
        """Slam::LoadMapsFromPCD; time < 0: the wall clock.  Returns the points read per type (-1: no file)"""
        self._check(self.L.lsa_slam_load_maps_pcd(self.h, os.fsencode(prefix), int(reset_maps), float(time)), "lsa_slam_load_maps_pcd")
        return self.map_io_counts()

    def target_submap(self, ktype):
        """Slam::GetTargetSubMap(k)"""
        n = self._check(self.L.lsa_slam_get_target_submap(self.h, ktype, None, 0), "lsa_slam_get_target_submap")
        out = np.zeros(max(n, 1), POINT_DTYPE)
        n = self.L.lsa_slam_get_target_submap(self.h, ktype, ptr(out), out.size)
        return out[:n].copy()

    def keypoints(self, ktype, which=0, cap=400000):
        """which: 0 undistorted BASE, 1 WORLD, 2 raw BASE."""
        out = np.zeros(cap, POINT_DTYPE)
        n = self._check(self.L.lsa_slam_get_keypoints(self.h, ktype, which, ptr(out), cap), "lsa_slam_get_keypoints")
        return out[:n].copy()

    def registered_frame(self, cap=None):
        cap = cap or max(self._n, 1 << 19)
        out = np.zeros(cap, POINT_DTYPE)
        n = self._check(self.L.lsa_slam_get_registered_frame(self.h, ptr(out), cap), "lsa_slam_get_registered_frame")
        return out[:n]

    def match_status(self, localization, ktype, cap=400000):
        st = np.zeros(cap, np.uint8)
        w = np.zeros(cap)
        n = self.L.lsa_slam_get_match_status(self.h, int(localization), ktype, ptr(st), ptr(w), cap)
        return st[:n].copy(), w[:n].copy()

    def stats(self):
        o = np.zeros(16)
        self.L.lsa_slam_get_stats(self.h, ptr(o))
        return o

    def context(self):
        return Context(handle=C.c_void_p(self.L.lsa_slam_context(self.h)))

    # ---- the keypoint log ("LoggingTimeout" != 0) and a corrected trajectory brought back
    def logged_frames(self):
        """frames in the keypoint log: one per logged pose while logging is on"""
        return self._check(self.L.lsa_slam_logged_frames(self.h), "lsa_slam_logged_frames")

    def logged_keypoints(self, frame, ktype):
        """the raw keypoints (BASE, not undistorted) logged with pose `frame` of the trajectory"""
        n = self._check(self.L.lsa_slam_get_logged_keypoints(self.h, frame, ktype, None, 0), "lsa_slam_get_logged_keypoints")
        out = np.zeros(max(n, 1), POINT_DTYPE)
        n = self._check(self.L.lsa_slam_get_logged_keypoints(self.h, frame, ktype, ptr(out), out.size), "lsa_slam_get_logged_keypoints")
        return out[:n].copy()

    def set_trajectory(self, poses, times):
        """what Slam::RunPoseGraphOptimization does after its optimizer: the logged poses replaced by poses (n, 4, 4) dated
        times (n,) -- those of trajectory() --, the maps rebuilt from the keypoint log under them.  Raises LsaError (its
        .code is E_STATE or E_ARG) and changes nothing when it cannot."""
        P = np.asarray(poses, np.float64).reshape(-1, 16)
        rows = np.ascontiguousarray(np.concatenate([P, np.asarray(times, np.float64).reshape(-1, 1)], axis=1))
        self._check(self.L.lsa_slam_set_trajectory_and_rebuild_maps(self.h, ptr(rows), rows.shape[0]), "lsa_slam_set_trajectory_and_rebuild_maps")


    def register_logged_frames(self, query, revisited, params=None, guess=None):
        """Loop closure: logged frame `query` registered against the logged keypoints around logged frame `revisited`
        (indices into trajectory()) -> LoopClosureResult.  params: a LoopClosureParams (None: its defaults); guess: (4, 4)
        world pose of query's BASE to start from (None: the logged pose).  The frame path does not notice the call.  Raises
        LsaError (.code E_STATE or E_ARG) and changes nothing when it cannot."""
        p = params if params is not None else LoopClosureParams()
        g = None if guess is None else np.ascontiguousarray(np.asarray(guess, np.float64).reshape(16))
        r = LoopClosureResultStruct()
        self._check(self.L.lsa_slam_register_logged_frames(self.h, int(query), int(revisited), C.byref(p), None if g is None else ptr(g), C.byref(r)),
                    "lsa_slam_register_logged_frames")
        return LoopClosureResult(r)

    def optimize_trajectory(self, loop_edges, apply=False, params=None, **kw):
        """Pose-graph optimization of the logged trajectory on the device (lsa_slam_optimize_logged_trajectory): the odometry
        chain of the log, pose 0 fixed, plus loop_edges -- (revisited, query, relative (4, 4), information (6, 6)) each, e.g.
        from register_logged_frames: (r, q, res.relative, information_from_covariance(res.covariance)).  apply=True hands the
        result to set_trajectory.  kw: PoseGraphParams' fields (odometry_information, odometry_sigma, ...).
        -> (poses (n, 4, 4), times (n,), PoseGraphResult)"""
        p = params if params is not None else PoseGraphParams(**kw)
        p.apply = int(bool(apply))
        E = pose_graph_edges(loop_edges)
        n = self._check(self.L.lsa_slam_logged_frames(self.h), "lsa_slam_logged_frames")
        rows = np.zeros((max(n, 1), 17))
        r = PoseGraphResultStruct()
        got = self._check(self.L.lsa_slam_optimize_logged_trajectory(self.h, ptr(E) if E.size else None, E.size, C.byref(p), ptr(rows), rows.shape[0], C.byref(r)),
                          "lsa_slam_optimize_logged_trajectory")
        return rows[:got, :16].reshape(-1, 4, 4).copy(), rows[:got, 16].copy(), PoseGraphResult(r)

    def run_pose_graph_optimization(self, gps_times, gps_xyz, gps_cov, gps_to_sensor=None, apply=True, time_offset=0.0, params=None, **kw):
        """Slam::RunPoseGraphOptimization (lsa_slam_run_pose_graph_optimization): the odometry chain of the log, every pose free,
        plus a position prior per GPS fix matched to a logged pose by time; solved on the device from the track laid onto the
        fixes, then brought back onto logged pose 0.  gps_times (G,), gps_xyz (G, 3), gps_cov (G, 3, 3); gps_to_sensor (4, 4):
        the antenna's pose in BASE (None: the identity).  apply=True hands the result to set_trajectory.  kw: PoseGraphParams'
        fields; odometry_information defaults to 1, the reference's rule.
        -> (poses (n, 4, 4), times (n,), gps_to_sensor (4, 4) = the optimized pose 0 in the GPS frame, PoseGraphResult, matches (G,))"""
        if params is None:
            kw.setdefault("odometry_information", 1)
        p = params if params is not None else PoseGraphParams(**kw)
        p.apply = int(bool(apply))
        t = np.ascontiguousarray(np.asarray(gps_times, np.float64).reshape(-1))
        x = np.ascontiguousarray(np.asarray(gps_xyz, np.float64).reshape(-1, 3))
        c = np.ascontiguousarray(np.asarray(gps_cov, np.float64).reshape(-1, 9))
        if not (x.shape[0] == c.shape[0] == t.size):
            raise _error("lsa_slam_run_pose_graph_optimization", E_ARG, "as many positions and covariances as times")
        cal = np.ascontiguousarray(np.asarray(np.eye(4) if gps_to_sensor is None else gps_to_sensor, np.float64).reshape(4, 4).copy())
        n = self._check(self.L.lsa_slam_logged_frames(self.h), "lsa_slam_logged_frames")
        rows = np.zeros((max(n, 1), 17))
        r = PoseGraphResultStruct()
        got = self._check(self.L.lsa_slam_run_pose_graph_optimization(self.h, ptr(t) if t.size else None, ptr(x) if t.size else None, ptr(c) if t.size else None, t.size,
                                                                      ptr(cal), float(time_offset), C.byref(p), ptr(rows), rows.shape[0], C.byref(r)),
                          "lsa_slam_run_pose_graph_optimization")
        times = rows[:got, 16].copy()
        return rows[:got, :16].reshape(-1, 4, 4).copy(), times, cal, PoseGraphResult(r), gps_match_trajectory(times, t, time_offset)

    def recognize_place(self, query, capacity=5, **params):
        """Place recognition: the logged frames before `query` that look like it -> [(frame, distance, shift, yaw)], best
        first.  params: PlaceSearch's fields (min_travelled, max_distance, max_descriptor_distance, exclusion_half_window)
        and PlaceParams' (rings, sectors, ...).  A start guess for register_logged_frames(query, frame) is
        P[frame] @ Rz(yaw).  The frame path does not notice the call.  Raises LsaError (.code E_STATE or E_ARG) when it cannot."""
        p = PlaceSearch(**params)
        out = (PlaceCandidateStruct * max(int(capacity), 1))()
        n = self._check(self.L.lsa_slam_recognize_place(self.h, int(query), C.byref(p), out, int(capacity)), "lsa_slam_recognize_place")
        return _candidates(out, n)


class RollingGrid:
    """LidarSlam::RollingGrid (RollingGrid.h:63-212) as the pipeline uses it: host code, no device involved."""

    def __init__(self, **params):
        self.L = lib()
        self.h = C.c_void_p(self.L.lsa_rolling_grid_create())
        if not self.h:
            raise LsaError("lsa_rolling_grid_create failed")
        for k, v in params.items():
            self.set(k, v)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.lsa_rolling_grid_destroy(self.h)
            self.h = None

    def set(self, name, value):
        if self.L.lsa_rolling_grid_set(self.h, name.encode(), float(value)) != 0:
            raise LsaError(f"lsa_rolling_grid_set({name}, {value}) refused")

    def reset(self, position=None):
        pos = None if position is None else np.ascontiguousarray(position, np.float32)
        self.L.lsa_rolling_grid_reset(self.h, None if pos is None else ptr(pos))

    def clear(self):
        self.L.lsa_rolling_grid_clear(self.h)

    def size(self):
        return self.L.lsa_rolling_grid_size(self.h)

    def roll(self, mn, mx):
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        self.L.lsa_rolling_grid_roll(self.h, ptr(mn), ptr(mx))

    def add(self, pts, fixed=False, time=-1.0, roll=True):
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        if self.L.lsa_rolling_grid_add(self.h, ptr(pts) if pts.size else None, pts.size, int(fixed), float(time), int(roll)) != 0:
            raise LsaError("lsa_rolling_grid_add failed")

    def clear_old_points(self, time):
        self.L.lsa_rolling_grid_clear_old_points(self.h, float(time))

    def get(self, clean=False):
        out = np.zeros(max(self.size(), 1), POINT_DTYPE)
        n = self.L.lsa_rolling_grid_get(self.h, int(clean), ptr(out), out.size)
        return out[:n].copy()

    def build_submap(self, mn=None, mx=None, min_nb_points=-1):
        if mn is None:
            return self.L.lsa_rolling_grid_build_submap(self.h, None, None, -1)
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        return self.L.lsa_rolling_grid_build_submap(self.h, ptr(mn), ptr(mx), int(min_nb_points))

    def submap_valid(self):
        return bool(self.L.lsa_rolling_grid_submap_valid(self.h))

    def submap(self):
        out = np.zeros(max(self.size(), 1), POINT_DTYPE)
        n = self.L.lsa_rolling_grid_submap(self.h, ptr(out), out.size)
        return out[:n].copy()


class DeviceGrid:
    """LidarSlam::RollingGrid resident on the device (lsa_device_grid_*): same calls as RollingGrid, the map lives in the
    memory of `ctx` and its sub-map becomes a kNN target of that context."""

    def __init__(self, ctx, **params):
        self.L = lib()
        self.ctx = ctx
        h = C.c_void_p()
        vp, i32, f64 = C.c_void_p, C.c_int, C.c_double
        self.L.lsa_device_grid_create.argtypes = [vp, C.POINTER(vp)]
        self.L.lsa_device_grid_destroy.argtypes = [vp]
        self.L.lsa_device_grid_set.argtypes = [vp, C.c_char_p, f64]
        self.L.lsa_device_grid_get_param.argtypes = [vp, C.c_char_p]
        self.L.lsa_device_grid_get_param.restype = f64
        self.L.lsa_device_grid_reset.argtypes = [vp, vp]
        self.L.lsa_device_grid_clear.argtypes = [vp]
        self.L.lsa_device_grid_size.argtypes = [vp]
        self.L.lsa_device_grid_add.argtypes = [vp, vp, i32, i32, f64, i32]
        self.L.lsa_device_grid_add_keypoints.argtypes = [vp, i32, i32, vp, f64]
        self.L.lsa_device_grid_roll.argtypes = [vp, vp, vp]
        self.L.lsa_device_grid_clear_old_points.argtypes = [vp, f64]
        self.L.lsa_device_grid_get.argtypes = [vp, i32, vp, i32]
        self.L.lsa_device_grid_build_submap.argtypes = [vp, vp, vp, i32, i32, i32]
        self.L.lsa_device_grid_submap_valid.argtypes = [vp]
        self.L.lsa_device_grid_stage_keypoints.argtypes = [vp, i32, i32, vp]
        self.L.lsa_device_grid_add_staged.argtypes = [vp, f64]
        self.L.lsa_device_grid_build_submap_begin.argtypes = [vp, vp, vp, i32, i32, i32]
        self.L.lsa_device_grid_build_submap_begin_for_keypoints.argtypes = [vp, i32, i32, i32, i32]
        self.L.lsa_device_grid_build_submap_end.argtypes = [vp]
        self.L.lsa_device_grid_submap_ahead_begin.argtypes = [vp, i32, i32, i32]
        self.L.lsa_device_grid_submap_ahead_wait.argtypes = [vp]
        self.L.lsa_device_grid_submap_ahead_take.argtypes = [vp, i32, i32, i32, i32, vp]
        if self.L.lsa_device_grid_create(ctx.h, C.byref(h)) != 0:
            raise LsaError("lsa_device_grid_create failed")
        self.h = h
        for k, v in params.items():
            self.set(k, v)

    def close(self):
        if getattr(self, "h", None):
            if self.ctx.h:  # a grid must go before its context (include/lidarslam_amd.h); one that outlived it is dropped
                self.L.lsa_device_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise LsaError(f"{what} failed ({rc}): {self.L.lsa_last_error(self.ctx.h).decode()}")
        return rc

    def set(self, name, value):
        self._check(self.L.lsa_device_grid_set(self.h, name.encode(), float(value)), f"lsa_device_grid_set({name})")

    def get_param(self, name):
        return float(self.L.lsa_device_grid_get_param(self.h, name.encode()))

    def reset(self, position=None):
        pos = None if position is None else np.ascontiguousarray(position, np.float32)
        self._check(self.L.lsa_device_grid_reset(self.h, None if pos is None else ptr(pos)), "lsa_device_grid_reset")

    def clear(self):
        self._check(self.L.lsa_device_grid_clear(self.h), "lsa_device_grid_clear")

    def size(self):
        return self._check(self.L.lsa_device_grid_size(self.h), "lsa_device_grid_size")

    def roll(self, mn, mx):
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        self._check(self.L.lsa_device_grid_roll(self.h, ptr(mn), ptr(mx)), "lsa_device_grid_roll")

    def add(self, pts, fixed=False, time=-1.0, roll=True):
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        self._check(self.L.lsa_device_grid_add(self.h, ptr(pts) if pts.size else None, pts.size, int(fixed), float(time), int(roll)), "lsa_device_grid_add")

    def add_keypoints(self, kset, ktype, pose, time):
        self._check(self.L.lsa_device_grid_add_keypoints(self.h, kset, ktype, ptr(pose16(pose)), float(time)), "lsa_device_grid_add_keypoints")

    def stage_keypoints(self, kset, ktype, pose):
        self._check(self.L.lsa_device_grid_stage_keypoints(self.h, kset, ktype, ptr(pose16(pose))), "lsa_device_grid_stage_keypoints")

    def add_staged(self, time):
        """the insertion of what stage_keypoints read; any host thread"""
        self._check(self.L.lsa_device_grid_add_staged(self.h, float(time)), "lsa_device_grid_add_staged")

    def add_pcd(self, path, fixed=False, time=-1.0, roll=True):
        """RollingGrid::Add of a PCD file's cloud, converted on the device"""
        self._check(self.L.lsa_device_grid_add_pcd(self.h, os.fsencode(path), int(fixed), float(time), int(roll)), "lsa_device_grid_add_pcd")

    def save_pcd(self, path, fmt=PCD_BINARY, clean=False):
        """RollingGrid::Get(clean) into a PCD file; returns the points written (0 and no file for an empty map)"""
        return self._check(self.L.lsa_device_grid_save_pcd(self.h, os.fsencode(path), int(fmt), int(clean)), "lsa_device_grid_save_pcd")

    def pcd_io_times(self):
        o = np.zeros(8)
        self.L.lsa_pcd_io_times(self.ctx.h, ptr(o))
        return o

    def build_submap_begin_for_keypoints(self, box_type, min_nb_points, ktype=PLANE, slot=TARGET_MAP):
        """box of the keypoints of `box_type` as Context.keypoint_bboxes_begin left it on the device"""
        self._check(self.L.lsa_device_grid_build_submap_begin_for_keypoints(self.h, box_type, int(min_nb_points), slot, ktype), "lsa_device_grid_build_submap_begin_for_keypoints")

    def build_submap_end(self):
        return self._check(self.L.lsa_device_grid_build_submap_end(self.h), "lsa_device_grid_build_submap_end")

    def submap_ahead_begin(self, box_type, min_nb_points, ktype=PLANE):
        """the sub-map for the box Context.keypoint_bboxes_begin left on the device, ahead of time, into the spare target"""
        self._check(self.L.lsa_device_grid_submap_ahead_begin(self.h, box_type, int(min_nb_points), ktype), "lsa_device_grid_submap_ahead_begin")

    def submap_ahead_wait(self):
        return self._check(self.L.lsa_device_grid_submap_ahead_wait(self.h), "lsa_device_grid_submap_ahead_wait")

    def submap_ahead_take(self, box_type, min_nb_points, ktype=PLANE, slot=TARGET_MAP):
        """(size, taken): taken == 1 when the sub-map extracted ahead became target (slot, ktype)"""
        taken = C.c_int(0)
        n = self._check(self.L.lsa_device_grid_submap_ahead_take(self.h, box_type, int(min_nb_points), slot, ktype, C.byref(taken)), "lsa_device_grid_submap_ahead_take")
        return n, taken.value

    def clear_old_points(self, time):
        self._check(self.L.lsa_device_grid_clear_old_points(self.h, float(time)), "lsa_device_grid_clear_old_points")

    def get(self, clean=False, capacity=None):
        """RollingGrid::Get(clean); capacity: room for so many points (default: the voxels the map holds)"""
        if capacity is None:
            capacity = max(int(self.get_param("Voxels")), 1)
        out = np.zeros(capacity, POINT_DTYPE)
        n = self._check(self.L.lsa_device_grid_get(self.h, int(clean), ptr(out), out.size), "lsa_device_grid_get")
        return out[:n].copy()

    def build_submap(self, mn=None, mx=None, min_nb_points=-1, ktype=PLANE, slot=TARGET_MAP):
        """the sub-map becomes target (slot, ktype) of the context; returns its size"""
        if mn is None:
            return self._check(self.L.lsa_device_grid_build_submap(self.h, None, None, -1, slot, ktype), "lsa_device_grid_build_submap")
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        return self._check(self.L.lsa_device_grid_build_submap(self.h, ptr(mn), ptr(mx), int(min_nb_points), slot, ktype), "lsa_device_grid_build_submap")

    def submap_valid(self):
        return bool(self.L.lsa_device_grid_submap_valid(self.h))
