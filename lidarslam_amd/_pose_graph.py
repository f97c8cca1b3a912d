"""The pose graph: edge / prior records, parameters, the lsa_pgo_* calls on the host or a Context, GPS helpers."""
import ctypes as C

import numpy as np

from ._abi import E_ARG, _error, lib
from ._native import ptr

# lsa_pgo_edge_t as a numpy record: from -> to, the measured inv(P[from]) @ P[to] (row-major 4x4), its 6x6 information
PGO_EDGE_DTYPE = np.dtype([("from", np.int32), ("to", np.int32), ("relative", np.float64, (16,)), ("information", np.float64, (36,))])
PGO_EDGE_BLOCK = 120  # doubles of an edge's block record: Haa[36] Hab[36] Hbb[36] ga[6] gb[6]
# lsa_pgo_prior_t: a measured position of the point carried by `pose` behind the solve's offset, and its 3x3 information
PGO_PRIOR_DTYPE = np.dtype([("pose", np.int32), ("reserved", np.int32), ("position", np.float64, (3,)), ("information", np.float64, (9,))])
PGO_PRIOR_BLOCK = 42  # doubles of a prior's block record: Haa[36] ga[6]
PGO_MAX_ITERATIONS, PGO_GRADIENT, PGO_STEP, PGO_COST, PGO_LAMBDA_CEILING, PGO_LINEAR_SOLVER_FAILED = range(6)
# LSA_PGO_LOSS_*: the robust losses of lidarslam_amd/csrc/lsa_pose_graph.h (ROBUST LOSS)
PGO_LOSS_NONE, PGO_LOSS_HUBER, PGO_LOSS_GEMAN_MCCLURE, PGO_LOSS_TUKEY = range(4)


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


class PoseGraphRobust(C.Structure):
    """lsa_pgo_robust_t: edge_loss / edge_scale act on the masked edges, prior_loss / prior_scale on every prior (PGO_LOSS_*,
    scales in sigmas); the defaults are lsa_pgo_robust_init's: no loss, scale 1."""

    _fields_ = [("edge_loss", C.c_int32), ("prior_loss", C.c_int32), ("edge_scale", C.c_double), ("prior_scale", C.c_double)]

    def __init__(self, **kw):
        super().__init__()
        lib().lsa_pgo_robust_init(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError(f"PoseGraphRobust has no field {k!r}")
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


def _pgo_mask(mask, m, what):
    """the edge mask of a robust call: None (every edge), or m flags"""
    if mask is None:
        return None
    f = np.ascontiguousarray(np.asarray(mask).astype(np.uint8).reshape(-1))
    if f.size != m:
        raise _error(what, E_ARG, "as many mask flags as edges")
    return f


def _pgo_robust(robust, what):
    if not isinstance(robust, PoseGraphRobust):
        raise _error(what, E_ARG, "robust must be a PoseGraphRobust")
    return robust


def pose_graph_robust_rho(loss, scale, s):
    """(rho(s), w = rho'(s)) of one loss (PGO_LOSS_*) at `scale` sigmas: the function of lsa_pose_graph.h's ROBUST LOSS on its
    own (lsa_pgo_robust_rho_host); s a number or an array."""
    flat = np.ascontiguousarray(np.asarray(s, np.float64)).reshape(-1)
    rho, w = np.zeros(flat.size), np.zeros(flat.size)
    a, b = C.c_double(), C.c_double()
    for i, v in enumerate(flat):
        rc = lib().lsa_pgo_robust_rho_host(int(loss), float(scale), float(v), C.byref(a), C.byref(b))
        if rc < 0:
            raise _error("lsa_pgo_robust_rho_host", rc, "a loss outside 0..3, or a scale that is not finite and positive")
        rho[i], w[i] = a.value, b.value
    if np.ndim(s) == 0:
        return float(rho[0]), float(w[0])
    return rho.reshape(np.shape(s)), w.reshape(np.shape(s))


def pose_graph_solve_robust(poses, fixed, edges, robust, mask=None, ctx=None, params=None, priors=None, offset=None, **kw):
    """pose_graph_solve under robust losses (lsa_pgo_solve_robust[_host]): robust a PoseGraphRobust; mask (m,) flags selecting
    the edges edge_loss acts on (None: every edge); prior_loss acts on every prior.
    -> (poses (n, 4, 4), PoseGraphResult, edge_verdict (m, 2), prior_verdict (k, 2)): per constraint {chi2, weight} at the
    returned poses, weight 1 for a constraint that is not robustified."""
    name = "lsa_pgo_solve_robust" + ("_host" if ctx is None else "")
    rb = _pgo_robust(robust, name)
    p = params if params is not None else PoseGraphParams(**kw)
    r = PoseGraphResultStruct()
    P, f, E = _pgo_graph(poses, fixed, edges)
    if f is None:
        raise _error(name, E_ARG, "fixed flags are needed")
    mk = _pgo_mask(mask, E.size, name)
    pa, keep = _pgo_priors(priors, offset)
    out = np.zeros((P.shape[0], 4, 4))
    ev, pv = np.zeros((E.size, 2)), np.zeros((pa[1], 2))
    L = lib()
    args = ([] if ctx is None else [ctx.h]) + [ptr(P), P.shape[0], ptr(f), ptr(E) if E.size else None, E.size, None if mk is None else ptr(mk)] + pa + [
        C.byref(p), C.byref(rb), ptr(out), C.byref(r), ptr(ev) if ev.size else None, ptr(pv) if pv.size else None]
    rc = getattr(L, name)(*args)
    if rc < 0:
        raise _error(name, rc, "the graph, the parameters or the losses are outside the definition" if ctx is None else L.lsa_last_error(ctx.h).decode())
    return out, PoseGraphResult(r), ev, pv


def pose_graph_linearize_robust(poses, edges, robust, mask=None, ctx=None):
    """-> e (m, 6), blocks (m, 120) (each record times its weight), chi2 (m,) (raw), rho (m,), w (m,): k_pgo_linearize_robust
    with a Context, its host twin without."""
    name = "lsa_pgo_linearize_robust" + ("_host" if ctx is None else "")
    rb = _pgo_robust(robust, name)
    P, _, E = _pgo_graph(poses, None, edges)
    mk = _pgo_mask(mask, E.size, name)
    m = E.size
    outs = [np.zeros((m, 6)), np.zeros((m, PGO_EDGE_BLOCK)), np.zeros(m), np.zeros(m), np.zeros(m)]
    L = lib()
    args = ([] if ctx is None else [ctx.h]) + [ptr(P), P.shape[0], ptr(E) if m else None, m, None if mk is None else ptr(mk), C.byref(rb)] + [ptr(o) for o in outs]
    rc = getattr(L, name)(*args)
    if rc < 0:
        raise _error(name, rc, L.lsa_last_error(ctx.h).decode() if ctx is not None else "the graph or the losses are outside the definition")
    return tuple(outs)


def pose_graph_linearize_priors_robust(poses, priors, robust, offset=None, ctx=None):
    """-> e (k, 3), blocks (k, 42) (each record times its weight), chi2 (k,), rho (k,), w (k,) of the position priors under
    robust.prior_loss: k_pgo_linearize_priors_robust with a Context, its host twin without."""
    name = "lsa_pgo_linearize_robust_priors" + ("_host" if ctx is None else "")
    rb = _pgo_robust(robust, name)
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    pa, keep = _pgo_priors(priors, offset)
    k = pa[1]
    outs = [np.zeros((k, 3)), np.zeros((k, PGO_PRIOR_BLOCK)), np.zeros(k), np.zeros(k), np.zeros(k)]
    L = lib()
    rc = getattr(L, name)(*([] if ctx is None else [ctx.h]), ptr(P), P.shape[0], *pa, C.byref(rb), *[ptr(o) for o in outs])
    if rc < 0:
        raise _error(name, rc, L.lsa_last_error(ctx.h).decode() if ctx is not None else "a prior or the losses are outside the definition")
    return tuple(outs)


def optimize_trajectory_robust(slam, loop_edges, robust, apply=False, params=None, **kw):
    """Slam.optimize_trajectory under robust.edge_loss on the caller's loop edges (lsa_slam_optimize_logged_trajectory_robust);
    the odometry chain is never discounted.  -> (poses (n, 4, 4), times (n,), PoseGraphResult, loop_verdict (m, 2) =
    {chi2, weight} per loop edge at the returned poses)"""
    name = "lsa_slam_optimize_logged_trajectory_robust"
    rb = _pgo_robust(robust, name)
    p = params if params is not None else PoseGraphParams(**kw)
    p.apply = int(bool(apply))
    E = pose_graph_edges(loop_edges)
    n = slam._check(slam.L.lsa_slam_logged_frames(slam.h), "lsa_slam_logged_frames")
    rows = np.zeros((max(n, 1), 17))
    verdict = np.zeros((E.size, 2))
    r = PoseGraphResultStruct()
    got = slam._check(getattr(slam.L, name)(slam.h, ptr(E) if E.size else None, E.size, C.byref(p), C.byref(rb), ptr(rows), rows.shape[0], C.byref(r),
                                            ptr(verdict) if E.size else None), name)
    return rows[:got, :16].reshape(-1, 4, 4).copy(), rows[:got, 16].copy(), PoseGraphResult(r), verdict


class LoopReportStruct(C.Structure):
    """lsa_loop_report_t."""

    _fields_ = [
        ("query", C.c_int32), ("frame", C.c_int32), ("distance", C.c_float), ("status", C.c_int32), ("yaw", C.c_double), ("iterations", C.c_int32),
        ("edge", C.c_int32), ("position_error", C.c_double), ("chi2", C.c_double), ("weight", C.c_double),
    ]


class LoopReport:
    """What close_loops says of one candidate: query, frame, distance (float32, of the descriptors), yaw [rad], status (the
    registration's: 0 registered, 1 too few matches, < 0 an E_* code), iterations, position_error [m], edge (its index among
    the loop edges, -1: none came of it), chi2 and weight (its verdict at the returned poses; 0 and -1 without an edge)."""

    def __init__(self, r):
        for name, _ in LoopReportStruct._fields_:
            setattr(self, name, getattr(r, name))
        self.distance = np.float32(r.distance)

    def __repr__(self):
        return f"LoopReport({self.__dict__})"


def close_loops(slam, robust=None, loop_params=None, apply=False, params=None, first_query=0, last_query=-1, query_stride=1, per_query=1, **search):
    """Finds every loop closure of the logged drive and closes them (lsa_slam_close_loops): detect_loop_closures, then
    register_logged_frames(query, frame, loop_params, P[frame] @ Rz(yaw)) for every candidate under the logged poses, an edge
    (frame, query, relative, information_from_covariance(covariance)) for every registration with status 0 and a positive
    definite covariance, and one optimize_trajectory_robust over them; apply=True puts the result back and rebuilds the maps.
    robust: a PoseGraphRobust (None: no loss); loop_params: a LoopClosureParams; params: a PoseGraphParams; search:
    PlaceSearch's fields and PlaceParams'.  -> (poses (n, 4, 4), times (n,), PoseGraphResult, [LoopReport]).  Without a
    candidate or an edge nothing is solved or changed, and the result's message says so."""
    from ._place import LoopClosureParams, _loop_detect

    name = "lsa_slam_close_loops"
    rb = PoseGraphRobust() if robust is None else _pgo_robust(robust, name)
    p = params if params is not None else PoseGraphParams()
    p.apply = int(bool(apply))
    lp = loop_params if loop_params is not None else LoopClosureParams()
    n = slam._check(slam.L.lsa_slam_logged_frames(slam.h), "lsa_slam_logged_frames")
    d, _ = _loop_detect(name, max(n, 1), first_query, last_query, query_stride, per_query, search)
    reports = (LoopReportStruct * (len(d.queries) * d.per_query))()
    rows = np.zeros((max(n, 1), 17))
    r = PoseGraphResultStruct()
    got = slam._check(slam.L.lsa_slam_close_loops(slam.h, C.byref(d), C.byref(lp), C.byref(p), C.byref(rb), ptr(rows), rows.shape[0], C.byref(r), reports, len(reports)), name)
    return rows[:n, :16].reshape(-1, 4, 4).copy(), rows[:n, 16].copy(), PoseGraphResult(r), [LoopReport(x) for x in reports[:got]]


def run_pose_graph_optimization_robust(slam, gps_times, gps_xyz, gps_cov, robust, gps_to_sensor=None, apply=True, time_offset=0.0, params=None, **kw):
    """Slam.run_pose_graph_optimization under robust.prior_loss on the GPS priors (lsa_slam_run_pose_graph_optimization_robust).
    -> (poses (n, 4, 4), times (n,), gps_to_sensor (4, 4), PoseGraphResult, matches (G,), fix_verdict (G, 2) = {chi2, weight}
    per fix at the returned poses, weight -1 for a fix that matched no pose)"""
    name = "lsa_slam_run_pose_graph_optimization_robust"
    rb = _pgo_robust(robust, name)
    if params is None:
        kw.setdefault("odometry_information", 1)
    p = params if params is not None else PoseGraphParams(**kw)
    p.apply = int(bool(apply))
    t = np.ascontiguousarray(np.asarray(gps_times, np.float64).reshape(-1))
    x = np.ascontiguousarray(np.asarray(gps_xyz, np.float64).reshape(-1, 3))
    c = np.ascontiguousarray(np.asarray(gps_cov, np.float64).reshape(-1, 9))
    if not (x.shape[0] == c.shape[0] == t.size):
        raise _error(name, E_ARG, "as many positions and covariances as times")
    cal = np.ascontiguousarray(np.asarray(np.eye(4) if gps_to_sensor is None else gps_to_sensor, np.float64).reshape(4, 4).copy())
    n = slam._check(slam.L.lsa_slam_logged_frames(slam.h), "lsa_slam_logged_frames")
    rows = np.zeros((max(n, 1), 17))
    verdict = np.zeros((t.size, 2))
    r = PoseGraphResultStruct()
    got = slam._check(getattr(slam.L, name)(slam.h, ptr(t) if t.size else None, ptr(x) if t.size else None, ptr(c) if t.size else None, t.size, ptr(cal), float(time_offset),
                                            C.byref(p), C.byref(rb), ptr(rows), rows.shape[0], C.byref(r), ptr(verdict) if t.size else None), name)
    times = rows[:got, 16].copy()
    return rows[:got, :16].reshape(-1, 4, 4).copy(), times, cal, PoseGraphResult(r), gps_match_trajectory(times, t, time_offset), verdict


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
