"""Slam: the pipeline (LidarSlam::Slam) on one device."""
import ctypes as C
import os

import numpy as np

from ._abi import E_ARG, LsaError, _error, lib
from ._context import Context
from ._native import POINT_DTYPE, ptr
from ._pcd import PCD_BINARY
from ._place import LoopClosureParams, LoopClosureResult, LoopClosureResultStruct, PlaceCandidateStruct, PlaceSearch, _candidates
from ._pose_graph import PoseGraphParams, PoseGraphResult, PoseGraphResultStruct, gps_match_trajectory, pose_graph_edges
from ._sensors import SensorTerms

DEBUG_INFORMATION_NAMES = [
    "EgoMotion: edges used", "EgoMotion: planes used", "Localization: edges used", "Localization: planes used",
    "Localization: blobs used", "Localization: position error", "Localization: orientation error",
    "Confidence: overlap", "Confidence: comply motion limits", "latency",
]


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
        if L.lsa_pin_host_memory(ptr(pts), pts.nbytes) != 0:
            raise LsaError("lsa_pin_host_memory failed")

    @staticmethod
    def unpin_cloud(pts):
        L = lib()
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
