"""Context: the kernel-level C ABI of one device context, with the solve / ICP-link helpers and the self tests."""
import ctypes as C

import numpy as np

from ._abi import E_STATE, KNN_MAX, TARGET_MAP, TARGET_PREVIOUS, LsaError, SolveResult, _error, lib
from ._native import MATCH_NSTATUS, POINT_DTYPE, SET_WORKING, ExtractParams, KernelStat, pose16, ptr
from ._place import PlaceParams
from ._pose_graph import (
    pose_graph_assemble,
    pose_graph_linearize,
    pose_graph_linearize_priors,
    pose_graph_premultiply,
    pose_graph_reanchor,
    pose_graph_retract,
    pose_graph_solve,
    pose_graph_spmv,
    pose_graph_tridiagonal_solve,
)

DEBUG_NAMES = [
    "sin_angle", "saliency", "depth_gap", "intensity_gap", "edge_keypoint", "plane_keypoint", "blob_keypoint",
    "edge_validity", "plane_validity", "blob_validity",
]


def icp_link_expected(x6, skipped, successful_steps, link):
    """lsa_icp_link_expected: (the 64 words of the block, the motion afterwards) as the host's arithmetic gives them"""
    words, motion = np.zeros(64, np.uint64), np.zeros(16, np.float64)
    x = np.ascontiguousarray(x6, np.float64)
    L = lib()
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


LM_STEP_RECORD, LM_STEP_RESULT = 42, 45  # doubles of lsa_selftest_lm_step's record and result (include/lidarslam_amd.h)


def selftest_lm_step(scripts, ctx=None):
    """lsa_selftest_lm_step (ctx: the device's step) or lsa_selftest_lm_host (ctx None: the host loop, no device) on
    scripts [(two_d, max_iter, min_matches, x0[6], sums (K, 29))] -> ([records (K, 42)], results (n, 45), status (n, 2))"""
    header = np.ascontiguousarray([(int(t), int(mi), int(mm), len(s)) for t, mi, mm, _x, s in scripts], np.int32).reshape(-1, 4)
    x0 = np.ascontiguousarray([x for _t, _mi, _mm, x, _s in scripts], np.float64).reshape(-1, 6)
    sums = np.ascontiguousarray(np.concatenate([np.asarray(s, np.float64).reshape(-1, 29) for *_h, s in scripts]))
    n, total = header.shape[0], sums.shape[0]
    records, results, status = np.zeros((total, LM_STEP_RECORD)), np.zeros((n, LM_STEP_RESULT)), np.zeros((n, 2), np.int32)
    L = lib()
    if ctx is None:
        rc = L.lsa_selftest_lm_host(n, ptr(header), ptr(x0), ptr(sums), ptr(records), ptr(results), ptr(status))
    else:
        rc = L.lsa_selftest_lm_step(ctx.h, n, ptr(header), ptr(x0), ptr(sums), ptr(records), ptr(results), ptr(status))
    if rc < 0:
        raise LsaError(f"lsa_selftest_lm_{'host' if ctx is None else 'step'} failed ({rc})" + (f": {L.lsa_last_error(ctx.h).decode()}" if ctx is not None else ""))
    ends = np.cumsum(header[:, 3])
    return [records[e - k:e] for e, k in zip(ends, header[:, 3])], results, status


def _profile(L, h):
    buf = (KernelStat * 64)()
    n = L.lsa_profile_get(h, buf, 64)
    return [
        {"name": buf[i].name.decode(), "launches": buf[i].launches, "total_ms": buf[i].total_ms, "bytes": buf[i].bytes}
        for i in range(max(n, 0))
    ]


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
        args = []
        for a in arrs:
            args += [a.ctypes.data_as(C.c_void_p), codes[a.dtype]]
        rc = self._check(f(self.h, arrs[1].size, *args, ptr(mp) if mp is not None else None, 0 if mp is None else mp.size, C.c_double(time_to_seconds),
                           C.byref(stamp), C.byref(kept)), "lsa_upload_polydata_frame")
        return stamp.value, kept.value, rc == 1

    def download_frame(self):
        """lsa_download_frame: the current frame as the device holds it, bit for bit"""
        out = np.zeros(max(self.L.lsa_frame_size(self.h), 1), POINT_DTYPE)
        n = self._check(self.L.lsa_download_frame(self.h, ptr(out), out.size), "lsa_download_frame")
        return out[:n]

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
        self._check(self.L.lsa_match_route_stats(self.h, ktype, ptr(out)), "lsa_match_route_stats")
        return out

    def match_trace(self, blocks):
        out = np.zeros((blocks, 12), np.uint64)
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
        self._check(self.L.lsa_solve_device_begin(self.h, type_mask, None if w is None else ptr(w), int(two_d), max_iter, min_matches), "lsa_solve_device_begin")

    def solve_device_end(self):
        """lsa_solve_device_end -> SolveResult, or the negative code (LSA_E_STATE ...) when there is none"""
        r = SolveResult()
        rc = self.L.lsa_solve_device_end(self.h, C.byref(r))
        return r if rc == 0 else rc

    def solve_device_drop(self):
        self._check(self.L.lsa_solve_device_drop(self.h), "lsa_solve_device_drop")

    def icp_link(self):
        """lsa_icp_link: reserves the block the next linked solve leaves for the iteration behind it -> ticket"""
        return self._check(self.L.lsa_icp_link(self.h), "lsa_icp_link")

    def solve_device_begin_linked(self, type_mask, prior6, leave_ticket, link, max_iter=15, two_d=False, min_matches=0):
        w = None if prior6 is None else np.ascontiguousarray(prior6, np.float64)
        self._check(self.L.lsa_solve_device_begin_linked(self.h, type_mask, None if w is None else ptr(w), int(two_d), max_iter, min_matches, leave_ticket,
                                                         None if link is None else C.byref(link)), "lsa_solve_device_begin_linked")

    def icp_link_peek(self, ticket):
        out = np.zeros(64, np.uint64)
        self._check(self.L.lsa_icp_link_peek(self.h, ticket, ptr(out)), "lsa_icp_link_peek")
        return out

    def icp_cancel(self, ticket):
        self._check(self.L.lsa_icp_cancel(self.h, ticket), "lsa_icp_cancel")

    def icp_abandon(self):
        self._check(self.L.lsa_icp_abandon(self.h), "lsa_icp_abandon")

    def match_types_linked(self, type_mask, query_set, params, undistort=False, slot=TARGET_MAP):
        """lsa_match_types_linked: 0 enqueued behind the link reserved last, 1 this match cannot wait behind a link"""
        return self._check(self.L.lsa_match_types_linked(self.h, slot, type_mask, query_set, C.byref(params), int(undistort)), "lsa_match_types_linked")

    def profile_event_overhead_us(self):
        return float(self.L.lsa_profile_event_overhead_us(self.h))

    def debug_set(self, name, value):
        self._check(self.L.lsa_debug_set(self.h, name.encode(), int(value)), "lsa_debug_set")

    def solve_device_trace(self):
        out = np.zeros(12, np.uint64)
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
