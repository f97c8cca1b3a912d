"""Loop detection over the whole keypoint log on the device (lidarslam_amd/csrc/lsa_place_detect.hip): k_place_search_rows
(lsa_place_search.hip) through L.place_search_rows, k_place_select_rows through L.kplog_detect_loops, and L.detect_loop_closures / L.close_loops on
top of them.

The reference is always the host statement -- L.place_distance for the table, L.place_detect_host for the candidates, the calls
CloseLoops is made of for its result: agreement is byte for byte."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest
from loop_detect_cases import TRAJECTORIES, grid, trajectory
from test_cpp_api import build_example

pytestmark = pytest.mark.gpu

# rings, sectors, the other parameters: test_gpu_place.py's.  32 x 120 has two wavefronts a pair and two pairs in flight, the
# others four pairs in flight; 1 x 1 and 3 x 7 sit below every tile
SHAPES = [
    (1, 1, {}),
    (3, 7, dict(min_range=2.5, max_range=50.0, height_offset=1.25)),
    (20, 60, {}),
    (32, 120, dict(height_offset=-1.0)),
]
NLOG = 300
STRIDED = dict(first_query=0, last_query=-1, query_stride=37)   # 300 frames: rows of 0, 37, ... 296 entries
CHUNKED = dict(first_query=0, last_query=129, query_stride=3)   # 130 frames: 2752 pairs, at least three runs at 6000 bytes


def points(L, xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(xyz.shape[0], L.POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    return p


def three_ways(pts):
    return [pts[k::3].copy() for k in range(3)]


def ring_cloud(sectors_used, rings=(10.0, 30.0, 50.0)):
    """points at cell centres of a 60-sector layout, in the given sectors, the same heights in every sector"""
    out = []
    for j in sectors_used:
        a = -np.pi + (j + 0.5) * 2 * np.pi / 60
        out += [(r * np.cos(a), r * np.sin(a), 1.0 + i) for i, r in enumerate(rings)]
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def log_frames(L):
    """300 small frames, every case of the search among them: identical, empty, turned, periodic (tied shifts), random"""
    rng = np.random.default_rng(4242)

    def scene(n):
        return np.column_stack([rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(-3, 8, n)])

    base, periodic, half = scene(300), ring_cloud(range(60)), ring_cloud(range(0, 60, 2))
    frames = []
    for c in range(NLOG):
        kind = c % 8
        if kind == 0:
            xyz = base
        elif kind == 1:
            xyz = np.zeros((0, 3))
        elif kind == 2:  # the base turned about z by whole sectors of the 60-sector shape
            a = (c // 8 % 60) * 2 * np.pi / 60
            xyz = base @ np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]).T
        elif kind == 3:
            xyz = periodic
        elif kind == 4:
            xyz = half
        elif kind == 5:
            xyz = np.vstack([base[:150], scene(80)])
        else:
            xyz = scene(int(rng.integers(1, 250)))
        frames.append(three_ways(points(L, xyz)))
    return frames


@pytest.fixture(scope="module")
def log_ctx(L, gpu_ctx, log_frames):
    ctx = gpu_ctx
    ctx.kplog_clear()
    for fr in log_frames:
        ctx.kplog_append_points(fr)
    yield ctx
    ctx.debug_set("place_max_blocks", 0)
    ctx.debug_set("place_table_bytes", 0)
    ctx.kplog_clear()


@pytest.fixture(scope="module")
def host_rows(L, log_frames):
    """per shape the host statement's rows for the two query sets, computed once: {query: (distance, shift)}"""
    made = {}

    def get(rings, sectors, extra):
        if (rings, sectors) not in made:
            p = dict(rings=rings, sectors=sectors, type_mask=7, **extra)
            desc = [L.scan_descriptor(np.concatenate(fr), **p) for fr in log_frames]
            rows = {}
            for q in sorted(set(range(0, NLOG, STRIDED["query_stride"])) | set(range(0, CHUNKED["last_query"] + 1, CHUNKED["query_stride"]))):
                pairs = [L.place_distance(desc[q], desc[i], **p) for i in range(q)]
                rows[q] = (np.array([d for d, _ in pairs], np.float32), np.array([s for _, s in pairs], np.int32))
            made[(rings, sectors)] = rows
        return made[(rings, sectors)]

    return get


def same_rows(got, want, what):
    for q, d, s in got:
        assert d.size == q and s.size == q
        assert d.tobytes() == want[q][0].tobytes(), (what, q, np.flatnonzero(d.view(np.uint32) != want[q][0].view(np.uint32))[:8])
        assert np.array_equal(s, want[q][1]), (what, q, np.flatnonzero(s != want[q][1])[:8])


@pytest.mark.parametrize("rings,sectors,extra", SHAPES)
def test_rows_equal_the_host_statement_under_both_knobs(L, log_ctx, host_rows, rings, sectors, extra):
    ctx = log_ctx
    p = dict(rings=rings, sectors=sectors, type_mask=7, **extra)
    want = host_rows(rings, sectors, extra)
    try:
        # 300 frames, 7 workgroups: every one walks a long piece of the tiles, across rows; then the default
        for blocks in (7, 0):
            ctx.debug_set("place_max_blocks", blocks)
            got = L.place_search_rows(ctx, **STRIDED, **p)
            assert [q for q, _, _ in got] == list(range(0, NLOG, 37))
            same_rows(got, want, ("strided", blocks))
        # 130 frames: one run, then runs of at most 750 entries (at least three), with few and with many workgroups
        whole = L.place_search_rows(ctx, **CHUNKED, **p)
        same_rows(whole, want, "one run")
        for table_bytes, blocks, untiled in [(6000, 0, 0), (6000, 7, 0), (1, 3, 0), (0, 0, 1), (6000, 7, 1)]:  # (1 byte: a run per query)
            ctx.debug_set("place_table_bytes", table_bytes)
            ctx.debug_set("place_max_blocks", blocks)
            ctx.debug_set("place_untiled", untiled)  # the columns one at a time instead of four: the same table
            got = L.place_search_rows(ctx, **CHUNKED, **p)
            assert sum(q for q, _, _ in got) * 8 > 2 * 6000
            for a, b in zip(got, whole):
                assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), (table_bytes, blocks, untiled, a[0])
    finally:
        ctx.debug_set("place_max_blocks", 0)
        ctx.debug_set("place_table_bytes", 0)
        ctx.debug_set("place_untiled", 0)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 9])
def test_rows_of_short_logs(L, log_frames, n):
    """a log of one frame has no pair (and no launch); 2 and 3 sit below the pairs in flight (2 from 65 sectors on, 4 below), 4,
    5, 6 and 9 one below, at and above them -- with every query, and with a single one, so that a row ends inside a tile"""
    ctx = L.Context(0)
    try:
        for fr in log_frames[:n]:
            ctx.kplog_append_points(fr)
        for rings, sectors, extra in SHAPES:
            p = dict(rings=rings, sectors=sectors, type_mask=7, **extra)
            desc = [L.scan_descriptor(np.concatenate(fr), **p) for fr in log_frames[:n]]
            want = {}
            for q in range(n):
                pairs = [L.place_distance(desc[q], desc[i], **p) for i in range(q)]
                want[q] = (np.array([d for d, _ in pairs], np.float32), np.array([s for _, s in pairs], np.int32))
            got = L.place_search_rows(ctx, **p)
            assert [q for q, _, _ in got] == list(range(n))
            same_rows(got, want, ("short", n))
            same_rows(L.place_search_rows(ctx, first_query=n - 1, **p), want, ("short, last query alone", n))
    finally:
        ctx.close()


def test_rows_refusals_leave_the_outputs_alone(L, log_ctx):
    ctx = log_ctx
    n = ctx.kplog_size()
    d, s = np.full(64, 7.5, np.float32), np.full(64, -9, np.int32)
    for first, last, stride, params in [(-1, 3, 1, {}), (3, 2, 1, {}), (0, n, 1, {}), (0, 3, 0, {}), (0, 3, -2, {}), (0, 3, 1, dict(rings=0)), (0, 3, 1, dict(sectors=121)),
                                        (0, 3, 1, dict(type_mask=0)), (0, 3, 1, dict(max_range=float("nan")))]:
        p = L.PlaceParams(**params)
        rc = ctx.L.lsa_kplog_place_search_rows(ctx.h, C.byref(p), first, last, stride, L.ptr(d), L.ptr(s))
        assert rc == L.E_ARG and np.all(d == 7.5) and np.all(s == -9), (first, last, stride, params)
    assert ctx.L.lsa_kplog_place_search_rows(ctx.h, C.byref(L.PlaceParams()), 0, 3, 1, None, None) == L.E_ARG
    with pytest.raises(L.LsaError) as e:
        L.place_search_rows(ctx, first_query=5, last_query=4)
    assert e.value.code == L.E_ARG


# ---- the selection -------------------------------------------------------------------------------------------------------------
def detect_both_ways(L, ctx, D, P, t, knobs, **case):
    want = L.place_detect_host(D, P, t, **case)
    for table_bytes, blocks in knobs:
        ctx.debug_set("place_table_bytes", table_bytes)
        ctx.debug_set("place_max_blocks", blocks)
        got = L.kplog_detect_loops(ctx, P, t, **case)
        assert got == want, (case, table_bytes, blocks, got[:4], want[:4])
    return want


@pytest.mark.parametrize("n,rings,sectors", [(40, 20, 60), (130, 3, 7), (130, 20, 60)])
def test_candidates_equal_the_host_statement_under_both_knobs(L, log_frames, n, rings, sectors):
    ctx = L.Context(0)
    seen = {"none": 0, "fewer": 0, "full": 0}
    try:
        for fr in log_frames[:n]:
            ctx.kplog_append_points(fr)
        p = dict(rings=rings, sectors=sectors, type_mask=7)
        assert ctx.kplog_describe(0, n - 1, **p) == n
        D = ctx.kplog_descriptors(0, n - 1, **p)
        for path in TRAJECTORIES:
            P, t = trajectory(path, n)
            for case in grid(n, 12):
                if (n, sectors) == (130, 60):  # (the host statement costs a tenth of a millisecond a pair here: the last twelve queries)
                    case["first_query"], case["last_query"] = 118, 129
                want = detect_both_ways(L, ctx, D, P, t, [(0, 0), (2000, 7)], **case, **p)
                assert ctx.kplog_described() == 0  # the store's laziness: everything was described before
                last = n - 1 if case["last_query"] < 0 else case["last_query"]
                for q in range(case["first_query"], last + 1, case["query_stride"]):
                    c = sum(1 for w in want if w[0] == q)
                    seen["none" if c == 0 else ("full" if c == case["per_query"] else "fewer")] += 1
        assert (n, sectors) == (130, 60) or (seen["none"] > 0 and seen["fewer"] > 0 and seen["full"] > 0), seen
        # a NaN pose: no frame passes a gate that cannot be decided, on either side
        P, t = trajectory("square", n)
        P[n // 2, 0, 3] = np.nan
        detect_both_ways(L, ctx, D, P, t, [(0, 0)], per_query=3, min_travelled=0.0, max_distance=2.5, exclusion_half_window=1, **p)
        detect_both_ways(L, ctx, D, P, t, [(0, 0)], per_query=3, min_travelled=3.0, exclusion_half_window=1, **p)
    finally:
        ctx.close()


def test_detection_refusals_write_nothing(L, log_frames):
    ctx = L.Context(0)
    try:
        for fr in log_frames[:6]:
            ctx.kplog_append_points(fr)
        P, t = trajectory("forward_back", 6)
        rows = np.ascontiguousarray(np.concatenate([P.reshape(-1, 16), t.reshape(-1, 1)], axis=1))
        out = (L.LoopCandidateStruct * 40)()
        before = bytes(out)
        for n, capacity, fields in [(6, 40, dict(query_stride=0)), (6, 40, dict(first_query=6)), (6, 40, dict(last_query=6)), (6, 40, dict(per_query=17)), (6, 40, dict(per_query=0)),
                                    (6, 5, {}), (6, 17, dict(per_query=3)), (5, 40, {}), (7, 40, {}), (6, 40, dict(rings=33)), (6, 40, dict(min_travelled=-1.0))]:
            d = L.LoopDetect(**fields)
            assert ctx.L.lsa_kplog_detect_loops(ctx.h, C.byref(d), L.ptr(rows), n, out, capacity) == L.E_ARG and bytes(out) == before, (n, capacity, fields)
        assert ctx.L.lsa_kplog_detect_loops(ctx.h, C.byref(L.LoopDetect()), None, 6, out, 40) == L.E_ARG
        assert ctx.L.lsa_kplog_detect_loops(ctx.h, C.byref(L.LoopDetect()), L.ptr(rows), 6, None, 40) == L.E_ARG
        assert L.kplog_detect_loops(ctx, P, t, min_travelled=0.0, per_query=16) == L.place_detect_host(ctx.kplog_descriptors(0, 5), P, t, min_travelled=0.0, per_query=16)
    finally:
        ctx.close()


# ---- Slam: detect_loop_closures and close_loops ----------------------------------------------------------------------------------
MODEL, SEED, FORWARD = 16, 1000, 12
ORDER = list(range(FORWARD)) + list(range(FORWARD - 2, -1, -1))


@pytest.fixture(scope="module")
def frames(L):
    return [L.synth_frame(MODEL, SEED, f) for f in range(FORWARD)]


def mapped(L, frames, upto=len(ORDER), **kw):
    """frames 0..11 forward, then the clouds 10..0 again with increasing stamps: the vehicle backs up over its own track"""
    s = L.Slam(0, EgoMotion=3, **{"LoggingTimeout": -1, **kw})
    period = frames[1][1] - frames[0][1]
    for f, c in enumerate(ORDER[:upto]):
        s.add_frame(frames[c][0], frames[0][1] + f * period, f)
    return s, period


@pytest.fixture(scope="module")
def revisit(L, frames):
    s, _ = mapped(L, frames)
    yield s
    s.close()


def snapshot(L, s):
    P, t, cov = s.trajectory()
    return (s.world_transform().tobytes(), s.covariance().tobytes(), [s.map(k).tobytes() for k in (L.EDGE, L.PLANE)], P.tobytes(), t.tobytes(), cov.tobytes(),
            s.logged_frames())


def test_detect_loop_closures_is_recognize_place_for_every_query(L, revisit):
    s = revisit
    n = s.logged_frames()
    before = snapshot(L, s)
    for search, descriptor in [
        (dict(min_travelled=2.0, max_distance=0.0, exclusion_half_window=2), {}),
        (dict(min_travelled=2.0, max_distance=1.0, exclusion_half_window=0), {}),
        (dict(min_travelled=0.0, max_distance=0.0, max_descriptor_distance=0.2, exclusion_half_window=1), dict(rings=32, sectors=120, type_mask=7)),
        (dict(min_travelled=1.0, exclusion_half_window=3), dict(rings=3, sectors=7, min_range=2.5, max_range=50.0, type_mask=2)),
    ]:
        for queries, per_query in [(dict(), 1), (dict(first_query=3, last_query=n - 2, query_stride=2), 4), (dict(first_query=n - 1), 16), (dict(query_stride=n + 1), 2)]:
            last = queries.get("last_query", n - 1)
            want = []
            for q in range(queries.get("first_query", 0), last + 1, queries.get("query_stride", 1)):
                want += [(q,) + c for c in s.recognize_place(q, capacity=per_query, **search, **descriptor)]
            # (the recognitions described every frame up to the last query: the detection describes none)
            got = L.detect_loop_closures(s, per_query=per_query, **queries, **search, **descriptor)
            assert s.context().kplog_described() == 0
            assert got == want, (search, descriptor, queries, per_query, got[:4], want[:4])
    assert len(L.detect_loop_closures(s, min_travelled=2.0, exclusion_half_window=2)) >= FORWARD - 4  # the way back revisits
    assert snapshot(L, s) == before
    for bad in [dict(first_query=n), dict(last_query=n), dict(first_query=-1), dict(first_query=5, last_query=4), dict(query_stride=0), dict(per_query=0), dict(per_query=17),
                dict(rings=0), dict(min_travelled=-1.0), dict(exclusion_half_window=-1)]:
        with pytest.raises(L.LsaError) as e:
            L.detect_loop_closures(s, **bad)
        assert e.value.code == L.E_ARG, bad
    out = (L.LoopCandidateStruct * 8)()
    assert s.L.lsa_slam_detect_loop_closures(s.h, C.byref(L.LoopDetect()), out, 8) == L.E_ARG  # room for fewer than queries * per_query


def test_detection_refuses_as_recognize_place_does(L, frames):
    off = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    for f in range(3):
        off.add_frame(frames[f][0], frames[f][1], f)
    with pytest.raises(L.LsaError) as e:
        L.detect_loop_closures(off, min_travelled=0.0)
    assert e.value.code == L.E_STATE and "LoggingTimeout" in str(e.value)
    with pytest.raises(L.LsaError) as e:
        L.close_loops(off, min_travelled=0.0)
    assert e.value.code == L.E_STATE and "LoggingTimeout" in str(e.value)
    off.set_param("LoggingTimeout", -1)
    for f in range(3, 5):
        off.add_frame(frames[f][0], frames[f][1], f)
    with pytest.raises(L.LsaError) as e:
        L.detect_loop_closures(off, min_travelled=0.0)
    assert e.value.code == L.E_STATE and "does not cover" in str(e.value)
    off.close()


def test_the_frame_path_does_not_notice_a_detection(L, frames):
    def run(detect):
        s, period = mapped(L, frames, upto=0)
        shots = []
        for f, c in enumerate(ORDER):
            s.add_frame(frames[c][0], frames[0][1] + f * period, f)
            if f in (14, 18):
                before = snapshot(L, s)
                if detect:
                    assert len(L.detect_loop_closures(s, min_travelled=1.0, exclusion_half_window=1, per_query=2)) >= 2
                    L.detect_loop_closures(s, min_travelled=0.0, rings=32, sectors=120, type_mask=7, first_query=f - 3)
                assert snapshot(L, s) == before
            if f >= 15:
                shots.append(snapshot(L, s))
        assert s.get_param("DeviceSolveFallbacks") == 0
        s.close()
        return shots

    assert run(True) == run(False)


def guess_of(P, yaw):
    """P * Rz(yaw) entry by entry as the library forms it: (a0 b0 + a1 b1) + a2 b2, the translation's sum closed by a3"""
    c, s = math.cos(yaw), math.sin(yaw)
    b = [[c, -s, 0.0, 0.0], [s, c, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    a = [[float(v) for v in row] for row in np.asarray(P, np.float64)]
    r = np.eye(4)
    for i in range(3):
        for j in range(3):
            r[i, j] = (a[i][0] * b[0][j] + a[i][1] * b[1][j]) + a[i][2] * b[2][j]
        r[i, 3] = ((a[i][0] * b[0][3] + a[i][1] * b[1][3]) + a[i][2] * b[2][3]) + a[i][3]
    return r


def by_hand(L, s, robust, lp, apply, **detect):
    """close_loops' definition, call by call -> (poses, result, verdicts, reports as tuples)"""
    P, t, _ = s.trajectory()
    found = L.detect_loop_closures(s, **detect)
    edges, reports = [], []
    for q, frame, distance, shift, yaw in found:
        reg = s.register_logged_frames(q, frame, lp, guess_of(P[frame], yaw))
        edge = -1
        if reg.status == 0:
            try:
                edges.append((frame, q, reg.relative, L.information_from_covariance(reg.covariance)))
                edge = len(edges) - 1
            except L.LsaError:
                pass
        reports.append([q, frame, distance, yaw, reg.status, reg.iterations, reg.position_error, edge])
    if not edges:
        return P, None, np.zeros((0, 2)), [tuple(r + [0.0, -1.0]) for r in reports]
    poses, times, res, verdict = L.optimize_trajectory_robust(s, edges, robust, apply=apply)
    assert np.array_equal(times, t)
    return poses, res, verdict, [tuple(r + ([verdict[r[7], 0], verdict[r[7], 1]] if r[7] >= 0 else [0.0, -1.0])) for r in reports]


def report_tuple(r):
    return (r.query, r.frame, r.distance, r.yaw, r.status, r.iterations, r.position_error, r.edge, r.chi2, r.weight)


def summary_tuple(res):
    return (res.initial_cost, res.final_cost, res.largest_step, res.final_lambda, res.iterations, res.accepted_steps, res.rejected_steps, res.pcg_iterations,
            res.last_pcg_iterations, res.pcg_truncated, res.termination, res.message)


DETECT = dict(min_travelled=2.0, max_distance=0.0, exclusion_half_window=2, first_query=FORWARD + 2, query_stride=4)


def false_one(s):
    """query 14 stands where frame 8 stood; with only frame 0 far enough back along the track to be admissible, its best match is
    a place eight frames away: a false candidate by construction, with max_descriptor_distance off.  The later queries 16 .. 22
    have the first frames to choose from and find where they are: true edges for the false one to contradict"""
    P, _, _ = s.trajectory()
    way = np.concatenate([[0.0], np.cumsum(np.linalg.norm(np.diff(P[:, :3, 3], axis=0), axis=1))])
    return dict(min_travelled=float(way[14] - way[1] / 2), max_distance=0.0, max_descriptor_distance=0.0, exclusion_half_window=2, first_query=14, last_query=22,
                query_stride=2)


def test_close_loops_is_its_definition(L, frames, revisit):
    s = revisit
    lp = L.LoopClosureParams(revisited_half_window=2)
    rb = L.PoseGraphRobust(edge_loss=L.PGO_LOSS_TUKEY, edge_scale=3.0)
    before = snapshot(L, s)
    FALSE_ONE = false_one(s)
    for detect in (DETECT, dict(DETECT, per_query=2, query_stride=5), FALSE_ONE):
        poses, times, res, reports = L.close_loops(s, rb, lp, **detect)
        hand_poses, hand_res, hand_verdict, hand_reports = by_hand(L, s, rb, lp, False, **detect)
        print("close_loops", detect, res, [report_tuple(r) for r in reports])
        assert [report_tuple(r) for r in reports] == hand_reports and len(reports) >= 1
        assert poses.tobytes() == hand_poses.tobytes()
        if hand_res is None:
            assert res.iterations == 0 and "nothing to solve" in res.message
        else:
            assert summary_tuple(res) == summary_tuple(hand_res)
        assert [r.edge for r in reports if r.edge >= 0] == list(range(hand_verdict.shape[0]))
        assert snapshot(L, s) == before and s.L.lsa_slam_last_error(s.h) in (None, b"")
    # the false candidate: a registered edge between places metres apart, disregarded under Tukey's loss
    poses, times, res, reports = L.close_loops(s, rb, lp, **FALSE_ONE)
    P, _, _ = s.trajectory()
    r = reports[0]
    apart = np.linalg.norm(P[r.frame][:3, 3] - P[r.query][:3, 3])
    step = np.linalg.norm(np.diff(P[:, :3, 3], axis=0), axis=1).mean()
    print("the false candidate:", report_tuple(r), "places", apart, "m apart, a frame is", step, "m")
    assert (r.query, r.frame) == (14, 0) and apart > 5 * step and r.edge == 0 and r.status == 0 and r.weight == 0.0
    assert len(reports) == 5 and all(x.edge >= 0 and x.weight > 0.5 for x in reports[1:])  # the others are believed
    # no candidate: nothing solved, nothing changed, no error text
    poses, times, res, reports = L.close_loops(s, rb, lp, min_travelled=1000.0)
    P, t, _ = s.trajectory()
    assert reports == [] and poses.tobytes() == P.tobytes() and np.array_equal(times, t) and res.iterations == 0 and "nothing to solve" in res.message
    assert snapshot(L, s) == before and s.L.lsa_slam_last_error(s.h) in (None, b"")
    # refusals are the composition's
    for bad in [dict(per_query=17), dict(first_query=s.logged_frames()), dict(rings=0)]:
        with pytest.raises(L.LsaError) as e:
            L.close_loops(s, rb, lp, **bad)
        assert e.value.code == L.E_ARG, bad
    with pytest.raises(L.LsaError) as e:
        L.close_loops(s, L.PoseGraphRobust(edge_loss=7), lp, **DETECT)
    assert e.value.code == L.E_ARG and snapshot(L, s) == before


def test_close_loops_applied_equals_the_hand_made_run(L, frames):
    lp = L.LoopClosureParams(revisited_half_window=2)
    rb = L.PoseGraphRobust(edge_loss=L.PGO_LOSS_HUBER, edge_scale=3.0)
    shots = []
    for hand in (False, True):
        s, period = mapped(L, frames)
        if hand:
            poses, res, _, _ = by_hand(L, s, rb, lp, True, **DETECT)
        else:
            poses, _, res, reports = L.close_loops(s, rb, lp, apply=True, **DETECT)
            assert any(r.edge >= 0 for r in reports)
        shot = [poses.tobytes(), summary_tuple(res), snapshot(L, s)]
        for k in range(2):  # frames go on afterwards
            s.add_frame(frames[1 + k][0], frames[0][1] + (len(ORDER) + k) * period, len(ORDER) + k)
            shot.append(snapshot(L, s))
        shots.append(shot)
        s.close()
    assert shots[0] == shots[1]
    P = np.frombuffer(shots[0][2][3], np.float64).reshape(-1, 4, 4)
    assert P.tobytes()[: len(shots[0][0])] == shots[0][0]  # applied: the logged poses are the optimized ones


def test_the_example_prints_a_report_that_matches_the_python_front_end(tmp_path, L, frames):
    exe = build_example(tmp_path, "slam_close_loops")
    r = subprocess.run([exe, str(MODEL), str(FORWARD)], capture_output=True, text=True, check=True)
    extra = {}
    for line in r.stdout.strip().splitlines():
        if line.startswith("#"):
            words = line.split()[1:]
            extra.setdefault(words[0], []).append([float(v) for v in words[1:]])
    s, period = mapped(L, frames)
    rb = L.PoseGraphRobust(edge_loss=L.PGO_LOSS_TUKEY, edge_scale=3.0)
    poses, _, res, reports = L.close_loops(s, rb, L.LoopClosureParams(revisited_half_window=2), apply=True, min_travelled=2.0, max_distance=0.0, exclusion_half_window=2,
                                           first_query=FORWARD + 2, query_stride=3)
    assert len(extra["loop"]) == len(reports) >= 2
    for line, rep in zip(extra["loop"], reports):
        assert [int(line[0]), int(line[1]), int(line[4]), int(line[5]), int(line[7])] == [rep.query, rep.frame, rep.status, rep.iterations, rep.edge]
        assert np.allclose(line[2:4] + [line[6]] + line[8:], [rep.distance, rep.yaw, rep.position_error, rep.chi2, rep.weight], rtol=1e-6, atol=1e-12)
    assert extra["solve"] == [[res.termination, res.iterations, res.pcg_iterations]]
    assert np.allclose(extra["cost"][0], [res.initial_cost, res.final_cost], rtol=1e-8, atol=0)
    assert np.allclose(extra["last"][0], poses[-1][:3, 3], atol=1e-9, rtol=0)
    for k in range(2):
        s.add_frame(frames[1 + k][0], frames[0][1] + (len(ORDER) + k) * period, len(ORDER) + k)
        assert np.allclose(extra["frame"][k], s.world_transform()[:3, 3], atol=1e-9, rtol=0)
    s.close()
