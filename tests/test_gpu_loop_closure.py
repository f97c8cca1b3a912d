"""Loop-closure registration of logged frames on the device: the ranged replay of the keypoint log (k_log_replay_range,
lsa_kplog_replay_range) and SlamCore::RegisterLoggedFrames on top of it.

The reference of the registration is stated here from oracle primitives alone, on the GPU Slam's own trajectory() and
logged_keypoints(): O.undistort / O.transform per logged frame (the sweep rule: pose i-1 at -(t[i] - t[i-1]), pose i at 0), a
fresh O.RollingGrid with the Slam's map parameters (add(roll=True), build_submap(None, None, -1), submap()), O.match per
type and O.lm_solve on the concatenated records per ICP iteration, O.covariance at the end.
Synthetic 16-ring sensor, seed 1000, 12 frames, EgoMotion = 3, LoggingTimeout = -1."""
import numpy as np
import pytest

from conftest import pose_diff

pytestmark = pytest.mark.gpu

MODEL, SEED, NFRAMES = 16, 1000, 12
LEAVES = {0: 0.30, 1: 0.60, 2: 0.30}  # Slam::Slam (Slam.cxx:143-161): edges, planes, blobs
ICP_MAX_ITER, LM_MAX_ITER, INIT_SAT, FINAL_SAT = 6, 15, 2.0, 0.5
BIG = np.finfo(np.float32).max


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def box_of(clouds):
    """min / max over all points of the clouds, a NaN coordinate taking no part; FLT_MAX / -FLT_MAX where there is none"""
    lo, hi = np.full(3, BIG, np.float32), np.full(3, -BIG, np.float32)
    for pts in clouds:
        for d, c in enumerate("xyz"):
            v = pts[c][~np.isnan(pts[c])]
            if v.size:
                lo[d], hi[d] = min(lo[d], v.min()), max(hi[d], v.max())
    return lo, hi


def replay_frame(O, pts, P, t, i, rule):
    """one logged frame under the poses P dated t: rule 0 rigid, 1 the rebuild's times (t[i] - t[i-1], 0), 2 the sweep's"""
    if pts.size == 0:
        return pts.copy()
    if rule == 0 or i == 0:
        return O.transform(pts, P[i])
    dt = t[i] - t[i - 1]
    return O.undistort(pts, P[i - 1], P[i], dt if rule == 1 else -dt, 0.0)


# ---- 1. the ranged replay at its awkward shapes (seam level) ---------------------------------------------------------------
EDGE_COUNTS = [5, 0, 1, 63, 0, 64, 65, 0, 257, 1000, 0, 40]
PLANE_COUNTS = [0, 700, 0, 1, 62, 0, 300, 0, 0, 64, 1, 0]
# (first, last): one frame with 1 / 63 / 64 / 65 / 257 edges; one frame without any keypoint; starting at frame 0; starting and
# ending on frames without edges; a frame without edges inside; the last frame alone; the whole log
RANGES = [(2, 2), (3, 3), (5, 5), (6, 6), (8, 8), (7, 7), (0, 3), (1, 4), (3, 5), (4, 7), (11, 11), (9, 11), (0, 11)]


@pytest.fixture(scope="module")
def seam_case(L):
    rng = np.random.default_rng(20261019)

    def cloud(n):
        p = np.zeros(n, L.POINT_DTYPE)
        for c in "xyz":
            p[c] = rng.uniform(-60, 60, n).astype(np.float32)
        p["w"] = 1.0
        p["time"] = rng.uniform(-0.1, 0.0, n)
        p["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
        p["laser_id"] = rng.integers(0, 16, n)
        return p

    log = [[cloud(e), cloud(p), cloud(0)] for e, p in zip(EDGE_COUNTS, PLANE_COUNTS)]  # no blobs at all
    P = [np.eye(4)]
    P[0][:3, :3] = rot(rng.normal(size=3), 0.3)
    P[0][:3, 3] = rng.uniform(-5, 5, 3)
    for _ in range(len(log) - 1):
        D = np.eye(4)
        D[:3, :3] = rot(rng.normal(size=3), rng.uniform(0.05, 0.3))
        D[:3, 3] = rng.uniform(-1, 1, 3)
        P.append(P[-1] @ D)
    t = 100.0 + 0.1 * np.arange(len(log)) + rng.uniform(0, 0.01, len(log))
    return log, np.array(P), t


@pytest.fixture(scope="module")
def seam_expected(O, seam_case):
    """per rule, type and frame the moved keypoints by the oracle: computed once"""
    log, P, t = seam_case
    return {rule: [[replay_frame(O, fr[k], P, t, i, rule) for i, fr in enumerate(log)] for k in range(3)] for rule in (0, 1, 2)}


@pytest.mark.parametrize("chunk_kib", [-1, 16])
def test_ranged_replay_at_awkward_shapes(L, gpu_ctx, seam_case, seam_expected, chunk_kib):
    log, P, t = seam_case
    ctx = gpu_ctx
    ctx.kplog_clear()
    ctx.debug_set("kplog_chunk_kib", chunk_kib)  # 16 KiB: the twelve frames (84 KB of points) take six chunks and more, the ranges cross them
    try:
        for fr in log:
            ctx.kplog_append_points(fr)
        assert ctx.kplog_size() == len(log)
        if chunk_kib > 0:
            assert ctx.kplog_bytes() >= 6 * (chunk_kib << 10)
        whole, _, _ = ctx.kplog_replay(P, t, undistort=True)
        for first, last in RANGES:
            for rule in (0, 1, 2):
                outs, mn, mx = ctx.kplog_replay_range(P, t, first, last, rule)
                for k in range(3):
                    exp = seam_expected[rule][k][first:last + 1]
                    want = np.concatenate(exp)
                    assert outs[k].size == want.size, (first, last, rule, k)
                    assert outs[k].tobytes() == want.tobytes(), (first, last, rule, k)
                    if rule == 1:  # the slice of the whole log's replay under the same poses
                        at = sum(fr[k].size for fr in log[:first])
                        assert outs[k].tobytes() == whole[k][at:at + want.size].tobytes(), (first, last, k)
                    lo, hi = box_of(exp)
                    assert mn[k].tobytes() == lo.tobytes() and mx[k].tobytes() == hi.tobytes(), (first, last, rule, k, mn[k], lo, mx[k], hi)
        # the totals this covers
        totals = {sum(EDGE_COUNTS[a:b + 1]) for a, b in RANGES} | {sum(PLANE_COUNTS[a:b + 1]) for a, b in RANGES}
        assert {0, 1, 63, 64, 65, 257} <= totals
        # a type left out of the mask comes out empty, with the box of an empty cloud
        outs, mn, mx = ctx.kplog_replay_range(P, t, 3, 6, 2, type_mask=2)
        assert outs[0].size == 0 and outs[1].size == sum(PLANE_COUNTS[3:7])
        assert np.all(mn[0] == BIG) and np.all(mx[0] == -BIG)
        # refusals, by argument: nothing is replayed
        n = len(log)
        for poses, times, first, last, rule, mask in [(P, t, -1, 2, 2, 7), (P, t, 3, 2, 2, 7), (P, t, 0, n, 2, 7), (P, t, n, n, 2, 7), (P[:-1], t[:-1], 0, 2, 2, 7),
                                                      (P, t, 0, 2, 3, 7), (P, t, 0, 2, -1, 7), (P, t, 0, 2, 2, 8)]:
            with pytest.raises(L.LsaError) as e:
                ctx.kplog_replay_range(poses, times, first, last, rule, type_mask=mask)
            assert e.value.code == L.E_ARG, (first, last, rule, mask)
        # the oldest frame dropped: frame indices move with the log
        ctx.kplog_pop_front()
        outs, _, _ = ctx.kplog_replay_range(P[1:], t[1:], 1, 2, 0)
        assert outs[0].tobytes() == np.concatenate(seam_expected[0][0][2:4]).tobytes()
    finally:
        ctx.kplog_clear()
        ctx.debug_set("kplog_chunk_kib", -1)


def test_nan_coordinates_take_no_part_in_the_box(L, O, gpu_ctx, seam_case):
    log, P, t = seam_case
    ctx = gpu_ctx
    ctx.kplog_clear()
    try:
        a, b = log[9][0][:70].copy(), log[1][1][:3].copy()
        a["x"][[0, 64, 69]] = np.nan  # a rigid pose mixes the coordinates: all three of the moved point are NaN
        b["y"][:] = np.nan            # a type whose every point is NaN
        ctx.kplog_append_points([a, b, log[0][2]])
        ctx.kplog_append_points([log[2][0], log[2][1], log[2][2]])
        outs, mn, mx = ctx.kplog_replay_range(P[:2], t[:2], 0, 0, 0)
        want = O.transform(a, P[0])
        ok = ~np.isnan(want["x"])
        assert ok.sum() == 67 and outs[0][ok].tobytes() == want[ok].tobytes()
        assert np.all(np.isnan(outs[0]["x"][~ok])) and np.all(np.isnan(outs[0]["z"][~ok]))
        lo, hi = box_of([want])
        assert mn[0].tobytes() == lo.tobytes() and mx[0].tobytes() == hi.tobytes()
        assert np.all(mn[1] == BIG) and np.all(mx[1] == -BIG) and np.all(mn[2] == BIG) and np.all(mx[2] == -BIG)
    finally:
        ctx.kplog_clear()


# ---- 2. the registration against a reference made of oracle primitives ------------------------------------------------------
@pytest.fixture(scope="module")
def frames(L):
    return [L.synth_frame(MODEL, SEED, f) for f in range(NFRAMES)]


@pytest.fixture(scope="module")
def mapped(L, frames):
    """the GPU Slam after the twelve frames, one per parameter set, with what the reference is built from: made once"""
    made = {}

    def get(**params):
        key = tuple(sorted(params.items()))
        if key not in made:
            s = L.Slam(0, **{**dict(EgoMotion=3, LoggingTimeout=-1), **params})
            for f, (pts, stamp) in enumerate(frames):
                s.add_frame(pts, stamp, f)
            P, t, _ = s.trajectory()
            assert P.shape[0] == NFRAMES == s.logged_frames()
            raw = [[s.logged_keypoints(i, k) for k in range(3)] for i in range(NFRAMES)]
            made[key] = (s, P, t, raw)
        return made[key]

    yield get
    for s, _, _, _ in made.values():
        s.close()


def rigid_inverse(T):
    """inv of a rigid pose as the library writes it: R^T, -(R^T t) summed left to right"""
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    for i in range(3):
        out[i, 3] = -((out[i, 0] * T[0, 3] + out[i, 1] * T[1, 3]) + out[i, 2] * T[2, 3])
    return out


def rigid_product(A, B):
    """A B of two rigid poses as the library writes it (sums left to right)"""
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = (A[i, 0] * B[0, j] + A[i, 1] * B[1, j]) + A[i, 2] * B[2, j]
        out[i, 3] = ((A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3]) + A[i, 2] * B[2, 3]) + A[i, 3]
    return out


def offset_guess(Pq, metres, degrees):
    """the logged pose moved by `metres` and turned by `degrees` in its own frame"""
    D = np.eye(4)
    D[:3, :3] = rot([0.2, -0.1, 1.0], np.deg2rad(degrees))
    D[:3, 3] = metres * np.array([0.6, 0.8, 0.0])
    return Pq @ D


def reference_registration(L, O, s, P, t, raw, q, r, wr, wq, guess):
    """RegisterLoggedFrames from oracle primitives alone"""
    n = len(P)
    types = [k for k, name in enumerate(("UseEdges", "UsePlanes", "UseBlobs")) if s.get_param(name)]
    rule = 2 if s.get_param("Undistortion") != 0 else 0
    r0, r1, q0, q1 = max(r - wr, 0), min(r + wr, n - 1), max(q - wq, 0), min(q + wq, n - 1)
    out = dict(target_points=np.zeros(3, np.int64), query_points=np.zeros(3, np.int64), first_histogram=np.zeros((3, 8), np.int32),
               last_histogram=np.zeros((3, 8), np.int32), status=0)
    # the target: the revisited frames under the logged trajectory, one Add into a fresh grid, the whole grid unfiltered
    target = {}
    for k in types:
        agg = np.concatenate([replay_frame(O, raw[i][k], P, t, i, rule) for i in range(r0, r1 + 1)])
        grid = O.RollingGrid(VoxelResolution=s.get_param("VoxelGridResolution"), GridSize=s.get_param("VoxelGridSize"), LeafSize=LEAVES[k],
                             Sampling=s.get_param("VoxelGridSamplingMode"), MinFramesPerVoxel=s.get_param("VoxelGridMinFramesPerVoxel"),
                             DecayingThreshold=s.get_param("VoxelGridDecayingThreshold"))
        grid.add(agg, fixed=False, time=-1.0, roll=True)
        grid.build_submap(None, None, -1)
        target[k] = grid.submap()
        out["target_points"][k] = target[k].size
    # the query: its frames under inv(P[q]) P[i], q's BASE frame
    inv = rigid_inverse(P[q])
    rel = np.array([rigid_product(inv, P[i]) for i in range(n)])
    query = {k: np.concatenate([replay_frame(O, raw[i][k], rel, t, i, rule) for i in range(q0, q1 + 1)]) for k in types}
    for k in types:
        out["query_points"][k] = query[k].size
    pose = np.array(guess, np.float64)
    iterations = 0
    for it in range(ICP_MAX_ITER):
        ratio = it / float(ICP_MAX_ITER - 1)
        sat = (1 - ratio) * INIT_SAT + ratio * FINAL_SAT
        mp = L.MatchParams.localization(saturation_distance=sat)
        status, records = [], []
        for k in types:
            st, _, rec, hist = O.match(query[k], target[k], k, mp, pose)
            status.append(st)
            records.append(rec)
            if it == 0:
                out["first_histogram"][k] = hist
            out["last_histogram"][k] = hist
        iterations += 1
        status, records = np.concatenate(status), np.concatenate(records)
        if int((status == 0).sum()) < s.get_param("MinNbMatchedKeypoints"):
            out["status"] = 1
            break
        pose, _, summary, _ = O.lm_solve(records, status, sat, pose, max_iter=LM_MAX_ITER, two_d=bool(s.get_param("TwoDMode")))
        if summary[0] == 1 or it + 1 == ICP_MAX_ITER:
            out["covariance"], out["errors"] = O.covariance(records, status, sat, pose)
            break
    out["world"], out["iterations"] = pose, iterations
    return out


CASES = [
    # q, r, wr, wq, guess offset [m], [deg], parameters of the Slam
    (9, 3, 2, 0, 0.0, 0.0, {}),
    (9, 3, 2, 0, 0.3, 1.0, {}),
    (9, 3, 2, 0, 1.0, 3.0, {}),
    (9, 1, 2, 0, 0.3, 1.0, {}),   # the window is clipped at frame 0, which is replayed rigidly
    (9, 3, 2, 1, 0.3, 1.0, {}),
    (11, 2, 1, 0, 0.5, 2.0, {}),
    (9, 3, 2, 0, 0.3, 1.0, {"Undistortion": 0}),
    (9, 3, 2, 0, 0.3, 1.0, {"MapsOnDevice": 0}),  # the scratch maps are device grids either way
]


@pytest.mark.parametrize("q,r,wr,wq,metres,degrees,params", CASES)
def test_registration_follows_the_oracle_composition(L, O, mapped, q, r, wr, wq, metres, degrees, params):
    s, P, t, raw = mapped(**params)
    guess = offset_guess(P[q], metres, degrees)
    ref = reference_registration(L, O, s, P, t, raw, q, r, wr, wq, guess)
    # conditions on the reference alone: a registration that did nothing cannot pass
    assert ref["status"] == 0
    print("reference: iterations", ref["iterations"], "last histogram", ref["last_histogram"].tolist(), "from the logged pose", pose_diff(P[q], ref["world"]))
    assert ref["last_histogram"][L.EDGE][0] >= 700 and ref["last_histogram"][L.PLANE][0] >= 2800, ref["last_histogram"]
    dp, da = pose_diff(P[q], ref["world"])
    assert dp < 0.05 and da < 0.01, (dp, da)

    lp = L.LoopClosureParams(revisited_half_window=wr, query_half_window=wq, icp_max_iter=ICP_MAX_ITER, lm_max_iter=LM_MAX_ITER,
                             init_saturation=INIT_SAT, final_saturation=FINAL_SAT)
    got = s.register_logged_frames(q, r, lp, None if metres == 0.0 and degrees == 0.0 else guess)
    print("device: iterations", got.iterations, "last histogram", got.last_histogram.tolist(), "from the reference", pose_diff(ref["world"], got.world))
    assert got.status == 0
    assert np.array_equal(got.target_points, ref["target_points"]), (got.target_points, ref["target_points"])
    assert np.array_equal(got.query_points, ref["query_points"]), (got.query_points, ref["query_points"])
    assert np.array_equal(got.first_histogram, ref["first_histogram"]), (got.first_histogram, ref["first_histogram"])
    dp, da = pose_diff(ref["world"], got.world)
    assert dp < 1e-7 and da < 1e-6, (dp, da)
    assert got.iterations == ref["iterations"]
    assert np.allclose(got.covariance, ref["covariance"], rtol=1e-5, atol=1e-12)  # as tests/test_gpu_pipeline.py holds the frames' covariances
    assert np.allclose([got.position_error, got.orientation_error], ref["errors"], rtol=1e-5)
    assert np.abs(got.relative - np.linalg.inv(P[r]) @ got.world).max() <= 1e-12


def test_default_parameters_are_the_localizations(L, mapped):
    s, P, t, raw = mapped()
    a = s.register_logged_frames(9, 3)
    b = s.register_logged_frames(9, 3, L.LoopClosureParams(revisited_half_window=5, icp_max_iter=int(s.get_param("LocalizationICPMaxIter")),
                                                           lm_max_iter=int(s.get_param("LocalizationLMMaxIter")), init_saturation=2.0, final_saturation=0.5), P[9])
    assert a.world.tobytes() == b.world.tobytes() and a.covariance.tobytes() == b.covariance.tobytes()
    assert np.array_equal(a.first_histogram, b.first_histogram) and np.array_equal(a.target_points, b.target_points)
    assert 1 <= a.iterations <= int(s.get_param("LocalizationICPMaxIter")) and a.status == 0


# ---- 3. the frame path does not notice ------------------------------------------------------------------------------------
def snapshot(L, s):
    P, t, cov = s.trajectory()
    return (s.world_transform().tobytes(), s.covariance().tobytes(), [s.map(k).tobytes() for k in (L.EDGE, L.PLANE)],
            [s.target_submap(k).tobytes() for k in (L.EDGE, L.PLANE)], P.tobytes(), t.tobytes(), cov.tobytes(), s.logged_frames(),
            s.get_param("NbrFrameProcessed"))


@pytest.mark.parametrize("on_device", [1, 0])
def test_the_frame_path_does_not_notice_a_registration(L, frames, on_device):
    def run(register):
        s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, MapsOnDevice=on_device)
        shots = []
        for f, (pts, stamp) in enumerate(frames):
            s.add_frame(pts, stamp, f)
            if f == 9:
                # (both runs read the same state through the same getters the same number of times: the registration and
                #  the refused calls are the only difference between them)
                before = snapshot(L, s)
                if register:
                    res = s.register_logged_frames(9, 3, L.LoopClosureParams(revisited_half_window=2))
                    assert res.status == 0 and res.target_points[L.PLANE] > 1000
                assert snapshot(L, s) == before
                # refused: the windows overlap, an index outside the log, a negative window
                for q, r, lp in [(9, 7, L.LoopClosureParams(revisited_half_window=2)), (9, 3, L.LoopClosureParams(revisited_half_window=2, query_half_window=4)),
                                 (10, 3, None), (9, -1, None), (9, 3, L.LoopClosureParams(revisited_half_window=-1))]:
                    if register:
                        with pytest.raises(L.LsaError) as e:
                            s.register_logged_frames(q, r, lp)
                        assert e.value.code == L.E_ARG, (q, r)
                    assert snapshot(L, s) == before
            if f >= 10:
                shots.append(snapshot(L, s))
        assert s.get_param("DeviceSolveFallbacks") == 0
        s.close()
        return shots

    assert run(True) == run(False)


def test_refusals_without_a_log(L, frames):
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    for f in range(3):
        s.add_frame(frames[f][0], frames[f][1], f)
    before = snapshot(L, s)
    with pytest.raises(L.LsaError) as e:
        s.register_logged_frames(1, 0, L.LoopClosureParams(revisited_half_window=0))
    assert e.value.code == L.E_STATE and "LoggingTimeout" in str(e.value)
    assert snapshot(L, s) == before
    s.close()
    # logging switched on after the first poses: the log does not cover them
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    for f in range(2):
        s.add_frame(frames[f][0], frames[f][1], f)
    s.set_param("LoggingTimeout", -1)
    for f in range(2, 5):
        s.add_frame(frames[f][0], frames[f][1], f)
    assert s.logged_frames() != s.trajectory()[1].size
    before = snapshot(L, s)
    with pytest.raises(L.LsaError) as e:
        s.register_logged_frames(4, 0, L.LoopClosureParams(revisited_half_window=0))
    assert e.value.code == L.E_STATE and "does not cover" in str(e.value)
    assert snapshot(L, s) == before
    s.close()


def test_a_stopped_log_refuses(L, gpu_ctx, seam_case, frames):
    log, P, t = seam_case
    ctx = gpu_ctx
    ctx.kplog_clear()
    try:
        ctx.debug_set("kplog_chunk_kib", 16)
        ctx.kplog_append_points(log[3])
        ctx.kplog_append_points(log[5])
        ctx.debug_set("kplog_fail_alloc", 1)
        with pytest.raises(L.LsaError):
            ctx.kplog_append_points(log[9])  # needs a chunk of its own, which cannot be had
        assert ctx.kplog_stopped() and ctx.kplog_size() == 2
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_replay_range(P[:2], t[:2], 0, 1, 2)
        assert e.value.code == L.E_STATE
    finally:
        ctx.debug_set("kplog_fail_alloc", 0)
        ctx.debug_set("kplog_chunk_kib", -1)
        ctx.kplog_clear()
    # the pipeline: logging stopped at the first frame, the frames went on
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    s.context().debug_set("kplog_fail_alloc", 1)
    s.add_frame(frames[0][0], frames[0][1], 0)
    s.context().debug_set("kplog_fail_alloc", 0)
    for f in (1, 2, 3):
        s.add_frame(frames[f][0], frames[f][1], f)
    before = snapshot(L, s)
    with pytest.raises(L.LsaError) as e:
        s.register_logged_frames(3, 0, L.LoopClosureParams(revisited_half_window=0))
    assert e.value.code == L.E_STATE and "stopped" in str(e.value)
    assert snapshot(L, s) == before
    s.close()


def test_too_few_matches_skip_the_registration(L, mapped):
    """below MinNbMatchedKeypoints: status 1, the pose is the guess, the one iteration that was matched is counted"""
    s, P, t, raw = mapped()
    guess = offset_guess(P[9], 0.3, 1.0)
    keep = s.get_param("MinNbMatchedKeypoints")
    s.set_param("MinNbMatchedKeypoints", 1000000)
    try:
        got = s.register_logged_frames(9, 3, L.LoopClosureParams(revisited_half_window=2, icp_max_iter=ICP_MAX_ITER), guess)
    finally:
        s.set_param("MinNbMatchedKeypoints", keep)
    assert got.status == 1 and got.iterations == 1
    assert got.world.tobytes() == guess.tobytes()
    assert np.abs(got.relative - np.linalg.inv(P[3]) @ guess).max() <= 1e-12
    assert got.first_histogram[L.PLANE][0] > 2000 and np.array_equal(got.first_histogram, got.last_histogram)
    assert np.all(got.covariance == 0)
    # and the next call registers again
    assert s.register_logged_frames(9, 3, L.LoopClosureParams(revisited_half_window=2), guess).status == 0
