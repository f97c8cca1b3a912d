"""Loop-closure candidates and place recognition: the parameter / result structs and the host statements."""
import ctypes as C

import numpy as np

from ._abi import E_ARG, _error, lib
from ._native import EDGE, PLANE, POINT_DTYPE, ptr


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


# ---- loop detection over the whole log (include/lidarslam_amd.h) ------------------------------------------------
MAX_PER_QUERY = 16  # candidates a query


class LoopDetect(C.Structure):
    """lsa_loop_detect_t: a PlaceSearch, the query set first_query, first_query + query_stride, ... <= last_query
    (last_query < 0: the last logged frame) and per_query (1..16) candidates a query."""

    _fields_ = [("search", PlaceSearch), ("first_query", C.c_int32), ("last_query", C.c_int32), ("query_stride", C.c_int32), ("per_query", C.c_int32)]

    def __init__(self, first_query=0, last_query=-1, query_stride=1, per_query=1, **search):
        super().__init__(PlaceSearch(**search), first_query, last_query, query_stride, per_query)

    @property
    def queries(self):
        return range(self.first_query, self.last_query + 1, self.query_stride)


class LoopCandidateStruct(C.Structure):
    """lsa_loop_candidate_t."""

    _fields_ = [("query", C.c_int32), ("frame", C.c_int32), ("shift", C.c_int32), ("distance", C.c_float), ("yaw", C.c_double)]


def _loop_candidates(out, n):
    """[(query, frame, distance, shift, yaw)]: distance a numpy float32, yaw a float [rad]"""
    return [(int(c.query), int(c.frame), np.float32(c.distance), int(c.shift), float(c.yaw)) for c in out[:n]]


def _loop_detect(what, n, first_query, last_query, query_stride, per_query, search):
    """-> (LoopDetect with last_query resolved on a log of n frames, room for its candidates); refuses what has no size"""
    d = LoopDetect(int(first_query), int(last_query), int(query_stride), int(per_query), **search)
    if d.last_query < 0:
        d.last_query = n - 1
    if not (n >= 1 and d.query_stride >= 1 and 0 <= d.first_query <= d.last_query < n and 1 <= d.per_query <= MAX_PER_QUERY):
        raise _error(what, E_ARG, "a query set outside the log, or per_query outside 1..16")
    return d, (LoopCandidateStruct * (len(d.queries) * d.per_query))()


def _rows17(poses, times):
    P = np.asarray(poses, np.float64).reshape(-1, 16)
    return np.ascontiguousarray(np.concatenate([P, np.asarray(times, np.float64).reshape(-1, 1)], axis=1))


def place_detect_host(descriptors, poses, times, first_query=0, last_query=-1, query_stride=1, per_query=1, **search):
    """The host statement of loop detection over a log (lsa_place_detect_host): descriptors (n, length) float32, poses
    (n, 4, 4) and times (n,) -> [(query, frame, distance, shift, yaw)], the queries ascending, each query's candidates best
    first: by definition place_select on the table of place_distance for every query of the set.  search: PlaceSearch's
    fields and PlaceParams'."""
    what = "lsa_place_detect_host"
    rows = _rows17(poses, times)
    n = rows.shape[0]
    d, out = _loop_detect(what, n, first_query, last_query, query_stride, per_query, search)
    D = np.ascontiguousarray(np.asarray(descriptors, np.float32).reshape(n, -1))
    if D.shape[1] != d.search.descriptor.length:
        raise _error(what, E_ARG, "descriptors of another shape than the parameters'")
    rc = lib().lsa_place_detect_host(C.byref(d), ptr(D), ptr(rows), n, out, len(out))
    if rc < 0:
        raise _error(what, rc, "parameters out of limits")
    return _loop_candidates(out, rc)


def place_search_rows(ctx, first_query=0, last_query=-1, query_stride=1, **params):
    """k_place_search_rows alone on the context's keypoint log (lsa_kplog_place_search_rows), no gates: per query of the set
    the (distance float32 (q,), shift int32 (q,)) of query q against the frames 0..q-1 -> [(query, distance, shift)]."""
    what = "lsa_kplog_place_search_rows"
    p = PlaceParams(**params)
    n = ctx.L.lsa_kplog_size(ctx.h)
    last = n - 1 if int(last_query) < 0 else int(last_query)
    if not (int(query_stride) >= 1 and 0 <= int(first_query) <= last < n):
        raise _error(what, E_ARG, "a query set outside the log")
    queries = list(range(int(first_query), last + 1, int(query_stride)))
    total = sum(queries)
    d, s = np.zeros(max(total, 1), np.float32), np.zeros(max(total, 1), np.int32)
    ctx._check(ctx.L.lsa_kplog_place_search_rows(ctx.h, C.byref(p), int(first_query), last, int(query_stride), ptr(d), ptr(s)), what)
    out, at = [], 0
    for q in queries:
        out.append((q, d[at:at + q], s[at:at + q]))
        at += q
    return out


def kplog_detect_loops(ctx, poses, times, first_query=0, last_query=-1, query_stride=1, per_query=1, **search):
    """Loop detection over the context's keypoint log (lsa_kplog_detect_loops: k_place_search_rows and k_place_select_rows per
    run of queries) under poses (n, 4, 4) dated times (n,) -> [(query, frame, distance, shift, yaw)] as place_detect_host."""
    what = "lsa_kplog_detect_loops"
    rows = _rows17(poses, times)
    d, out = _loop_detect(what, rows.shape[0], first_query, last_query, query_stride, per_query, search)
    return _loop_candidates(out, ctx._check(ctx.L.lsa_kplog_detect_loops(ctx.h, C.byref(d), ptr(rows), rows.shape[0], out, len(out)), what))


def detect_loop_closures(slam, first_query=0, last_query=-1, query_stride=1, per_query=1, **search):
    """Every place the logged drive revisited (lsa_slam_detect_loop_closures): slam.recognize_place(q, capacity=per_query)
    for every query of the set in one pass on the device -> [(query, frame, distance, shift, yaw)], the queries ascending,
    each query's candidates best first.  search: PlaceSearch's fields and PlaceParams'.  Raises LsaError (.code E_STATE or
    E_ARG) when it cannot."""
    what = "lsa_slam_detect_loop_closures"
    n = slam._check(slam.L.lsa_slam_logged_frames(slam.h), "lsa_slam_logged_frames")
    if n < 1:
        d, out = LoopDetect(int(first_query), int(last_query), int(query_stride), int(per_query), **search), (LoopCandidateStruct * 1)()
        return _loop_candidates(out, slam._check(slam.L.lsa_slam_detect_loop_closures(slam.h, C.byref(d), out, 0), what))  # (the library says why not)
    d, out = _loop_detect(what, n, first_query, last_query, query_stride, per_query, search)
    return _loop_candidates(out, slam._check(slam.L.lsa_slam_detect_loop_closures(slam.h, C.byref(d), out, len(out)), what))


# ---- place recognition against the maps: the map as seen from a viewpoint (include/lidarslam_amd.h) ----------
class MapPlaceSearch(C.Structure):
    """lsa_map_place_search_t: the descriptor's parameters and the selection's.  near_xyz is read only when max_distance > 0."""

    _fields_ = [
        ("descriptor", PlaceParams), ("max_descriptor_distance", C.c_double), ("exclusion_radius", C.c_double), ("near_xyz", C.c_double * 3),
        ("max_distance", C.c_double),
    ]

    def __init__(self, max_descriptor_distance=0.0, exclusion_radius=5.0, near_xyz=(0.0, 0.0, 0.0), max_distance=0.0, **descriptor):
        super().__init__(PlaceParams(**descriptor), max_descriptor_distance, exclusion_radius, (C.c_double * 3)(*[float(v) for v in near_xyz]), max_distance)


class MapPlaceCandidateStruct(C.Structure):
    """lsa_map_place_candidate_t."""

    _fields_ = [("viewpoint", C.c_int32), ("shift", C.c_int32), ("distance", C.c_float), ("reserved", C.c_float), ("yaw", C.c_double), ("guess", C.c_double * 16)]


class MapPlaceSummaryStruct(C.Structure):
    """lsa_map_place_summary_t."""

    _fields_ = [("viewpoints", C.c_int32), ("described", C.c_int32), ("map_points", C.c_int64 * 3), ("query_points", C.c_int64 * 3)]


def _map_candidates(out, n):
    """[(viewpoint, distance, shift, yaw, guess)]: distance a numpy float32, yaw a float [rad], guess (4, 4) float64"""
    return [(int(c.viewpoint), np.float32(c.distance), int(c.shift), float(c.yaw), np.array(c.guess, np.float64).reshape(4, 4)) for c in out[:n]]


def _as_points(points):
    pts = np.asarray(points)
    if pts.dtype != POINT_DTYPE:
        xyz = np.asarray(points, np.float32).reshape(-1, 3)
        pts = np.zeros(xyz.shape[0], POINT_DTYPE)
        pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    return np.ascontiguousarray(pts.reshape(-1))


def _as_viewpoints(viewpoints):
    return np.ascontiguousarray(np.asarray(viewpoints, np.float64).reshape(-1, 3))


def map_descriptor(points, viewpoint, **params):
    """The host statement of the descriptor of a map as seen from `viewpoint` (lsa_map_descriptor_host): points a POINT_DTYPE
    array, or (n, 3) xyz, of every map that takes part; viewpoint (3,) in the maps' frame -> float32 (rings * sectors +
    sectors,).  By definition scan_descriptor of the points translated as x = float32(float64(p.x) - v.x).  params:
    PlaceParams' fields."""
    p = PlaceParams(**params)
    pts = _as_points(points)
    v = np.ascontiguousarray(np.asarray(viewpoint, np.float64).reshape(-1))
    if v.size != 3:
        raise _error("lsa_map_descriptor_host", E_ARG, "a viewpoint is three coordinates")
    out = np.zeros(max(p.rings, 0) * max(p.sectors, 0) + max(p.sectors, 0), np.float32)
    rc = lib().lsa_map_descriptor_host(C.byref(p), ptr(pts) if pts.size else None, pts.size, ptr(v), ptr(out))
    if rc < 0:
        raise _error("lsa_map_descriptor_host", rc, "parameters out of limits or a viewpoint that is not finite")
    return out


def map_place_select(distance, shift, viewpoints, capacity=5, **search):
    """The host statement of the selection among viewpoints (lsa_map_place_select_host): distance / shift the table of the V
    viewpoints (V, 3) -> [(viewpoint, distance, shift, yaw, guess)], best first; guess = Translation(viewpoint) @ Rz(yaw).
    search: MapPlaceSearch's fields and PlaceParams' (of which the selection reads sectors)."""
    p = MapPlaceSearch(**search)
    vp = _as_viewpoints(viewpoints)
    d = np.ascontiguousarray(np.asarray(distance, np.float32).reshape(-1))
    s = np.ascontiguousarray(np.asarray(shift, np.int32).reshape(-1))
    if d.size != vp.shape[0] or s.size != vp.shape[0]:
        raise _error("lsa_map_place_select_host", E_ARG, "a table of another length than the viewpoints")
    out = (MapPlaceCandidateStruct * max(int(capacity), 1))()
    rc = lib().lsa_map_place_select_host(ptr(d) if d.size else None, ptr(s) if s.size else None, ptr(vp) if vp.size else None, vp.shape[0], p.descriptor.sectors,
                                         C.byref(p), out, int(capacity))
    if rc < 0:
        raise _error("lsa_map_place_select_host", rc, "bad argument")
    return _map_candidates(out, rc)


def map_place_describe(ctx, points_or_grids, viewpoints, **params):
    """Fills the context's table of map descriptors (k_map_describe): points_or_grids a POINT_DTYPE array (uploaded), or a
    sequence of three DeviceGrid / None, the maps by type, read where they live.  Returns how many viewpoints were described:
    all, or 0 when the grids, the viewpoints and the parameters are those of the table (it is kept)."""
    p = PlaceParams(**params)
    vp = _as_viewpoints(viewpoints)
    if isinstance(points_or_grids, (list, tuple)) and len(points_or_grids) == 3 and all(g is None or hasattr(g, "h") for g in points_or_grids):
        grids = (C.c_void_p * 3)(*[None if g is None else g.h for g in points_or_grids])
        return ctx._check(ctx.L.lsa_map_place_describe_grids(ctx.h, grids, C.byref(p), ptr(vp) if vp.size else None, vp.shape[0]), "lsa_map_place_describe_grids")
    pts = _as_points(points_or_grids)
    return ctx._check(ctx.L.lsa_map_place_describe_points(ctx.h, C.byref(p), ptr(pts) if pts.size else None, pts.size, ptr(vp) if vp.size else None, vp.shape[0]),
                      "lsa_map_place_describe_points")


def map_place_descriptors(ctx, first, last, out=None, **params):
    """slots first..last of the context's table -> float32 (last - first + 1, length); slot V, the query's, once a search
    has described it.  params: PlaceParams' fields as the table was made under (they give the length of a slot)."""
    count = max(int(last) - int(first) + 1, 1)
    if out is None:
        out = np.zeros((count, max(PlaceParams(**params).length, 1)), np.float32)
    ctx._check(ctx.L.lsa_map_place_descriptors(ctx.h, int(first), int(last), ptr(out)), "lsa_map_place_descriptors")
    return out


def map_place_search(ctx, kset, out=None, **params):
    """The keypoint set `kset` of the context against the table's V viewpoints (k_log_describe into the query's slot, then
    k_place_search) -> (distance float32 (V,), shift int32 (V,)), written into out = (distance, shift) where given."""
    p = PlaceParams(**params)
    v = ctx.L.lsa_map_place_viewpoints(ctx.h)
    d, s = out if out is not None else (np.zeros(max(v, 1), np.float32), np.zeros(max(v, 1), np.int32))
    ctx._check(ctx.L.lsa_map_place_search(ctx.h, C.byref(p), int(kset), ptr(d), ptr(s)), "lsa_map_place_search")
    return d[:v], s[:v]


def map_place_slices(ctx):
    """the slices of the table's last description -> float32 (slices, 4): min x, min y, max x, max y of each"""
    n = ctx._check(ctx.L.lsa_map_place_slices(ctx.h, None, 0), "lsa_map_place_slices")
    out = np.zeros((max(n, 1), 4), np.float32)
    ctx._check(ctx.L.lsa_map_place_slices(ctx.h, ptr(out), out.shape[0]), "lsa_map_place_slices")
    return out[:n]


class MapPlaceSummary:
    """What recognize_place_in_maps says beside the candidates: viewpoints, described (viewpoints this call described; 0: the
    table was kept), map_points / query_points (3,) per keypoint type."""

    def __init__(self, r):
        self.viewpoints, self.described = int(r.viewpoints), int(r.described)
        self.map_points = np.array(r.map_points, np.int64)
        self.query_points = np.array(r.query_points, np.int64)


def recognize_place_in_maps(slam, viewpoints=None, capacity=5, **search):
    """Place recognition against the maps (lsa_slam_recognize_place_in_maps): the viewpoints (V, 3), positions in the maps'
    frame, from which the maps look like the last frame -> ([(viewpoint, distance, shift, yaw, guess)], MapPlaceSummary), best
    first.  slam.set_world_transform_from_guess(guess) starts the localization there; the call itself moves nothing.
    viewpoints None: the positions of slam.trajectory().  search: MapPlaceSearch's fields and PlaceParams'.  Raises LsaError
    (.code E_STATE or E_ARG) when it cannot."""
    p = MapPlaceSearch(**search)
    if viewpoints is None:
        viewpoints = np.asarray(slam.trajectory()[0], np.float64).reshape(-1, 4, 4)[:, :3, 3]
        if viewpoints.shape[0] == 0:
            raise _error("lsa_slam_recognize_place_in_maps", E_ARG, "the trajectory is empty and no viewpoints were given")
    vp = _as_viewpoints(viewpoints)
    out = (MapPlaceCandidateStruct * max(int(capacity), 1))()
    summary = MapPlaceSummaryStruct()
    n = slam._check(slam.L.lsa_slam_recognize_place_in_maps(slam.h, ptr(vp) if vp.size else None, vp.shape[0], C.byref(p), out, int(capacity), C.byref(summary)),
                    "lsa_slam_recognize_place_in_maps")
    return _map_candidates(out, n), MapPlaceSummary(summary)
