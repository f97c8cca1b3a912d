"""The keypoint log in device memory and a corrected trajectory brought back into the library
(lsa_kplog.hip, SlamCore::SetTrajectoryAndRebuildMaps): what Slam::RunPoseGraphOptimization does after its optimizer
(slam_lib/src/Slam.cxx:404-477), stated from oracle primitives alone -- raw keypoints, O.undistort / O.transform, a
fresh oracle grid's add(roll=False) / roll / get -- and compared byte for byte.  Synthetic 16-ring sensor, 8 frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODEL, SEED, NFRAMES = 16, 1000, 8
LEAVES = {0: 0.30, 1: 0.60, 2: 0.30}  # Slam::Slam (Slam.cxx:143-161): edges, planes, blobs


@pytest.fixture(scope="module")
def frames(L):
    return [L.synth_frame(MODEL, SEED, f) for f in range(NFRAMES + 2)]


@pytest.fixture(scope="module")
def raw_keypoints(O, frames):
    """raw keypoints (BASE) of every frame and type by the oracle; they do not depend on the pose.  Computed once."""
    o = O.Slam(EgoMotion=3, UseBlobs=1)
    out = []
    for f, (pts, stamp) in enumerate(frames):
        o.add_frame(pts, stamp, f)
        out.append([o.keypoints(k, which=2) for k in range(3)])
    return out


def types_in_use(L, blobs):
    return (L.EDGE, L.PLANE, L.BLOB) if blobs else (L.EDGE, L.PLANE)


def rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def expected_replay(O, frames_k, P, t, undistort):
    """Slam.cxx:426-447 from oracle primitives: per frame the moved keypoints of one type"""
    out = []
    for i, pts in enumerate(frames_k):
        if undistort and i >= 1:
            out.append(O.undistort(pts, P[i - 1], P[i], t[i] - t[i - 1], 0.0) if pts.size else pts.copy())
        else:
            out.append(O.transform(pts, P[i]) if pts.size else pts.copy())
    return out


def box_of(pts):
    """pcl::getMinMax3D: FLT_MAX / -FLT_MAX for an empty cloud (what the oracle's MinMax3D gives)"""
    big = np.finfo(np.float32).max
    if pts.size == 0:
        return np.full(3, big, np.float32), np.full(3, -big, np.float32)
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1)
    return xyz.min(0), xyz.max(0)


# ---- 1. the log is the reference's log ---------------------------------------------------------------------------------
@pytest.mark.parametrize("timeout", [-1.0, 0.45, 0.0])
def test_the_log_is_the_references_log(L, O, frames, raw_keypoints, timeout):
    g, o = L.Slam(0, EgoMotion=3, LoggingTimeout=timeout), O.Slam(EgoMotion=3, LoggingTimeout=timeout)
    trimmed = False
    for f in range(NFRAMES):
        pts, stamp = frames[f]
        g.add_frame(pts, stamp, f)
        o.add_frame(pts, stamp, f)
        n = g.trajectory()[1].size
        assert n == o.trajectory()[1].size
        if timeout == 0.0:
            assert g.logged_frames() == 0 and g.get_param("LoggedKeypointsBytes") == 0
            continue
        assert g.logged_frames() == n
        trimmed = trimmed or n < f + 1
        for i in range(n):  # pose i of the trajectory is frame f + 1 - n + i
            for k in (L.EDGE, L.PLANE):
                ref = raw_keypoints[f + 1 - n + i][k]
                assert ref.size > 0
                if i == n - 1:
                    assert ref.tobytes() == o.keypoints(k, which=2).tobytes()  # (the shared reference is this oracle's too)
                assert g.logged_keypoints(i, k).tobytes() == ref.tobytes(), (f, i, k)
            assert g.logged_keypoints(i, L.BLOB).size == 0
    if timeout > 0:
        assert trimmed and g.logged_frames() < NFRAMES  # frames 0.1 s apart: the log was trimmed with the trajectory
    if timeout != 0.0:
        assert g.get_param("LoggedKeypointsBytes") >= sum(raw_keypoints[NFRAMES - 1][k].nbytes for k in (0, 1))
        g.reset(False)
        assert g.logged_frames() == n  # Reset(false) keeps the log, as the reference's resetLog does
        g.reset(True)
        assert g.logged_frames() == 0
    g.close()


def test_logging_storage_is_a_parameter_with_one_meaning(L):
    g = L.Slam(0)
    for v in range(5):  # PointCloudStorageType
        g.set_param("LoggingStorage", v)
        assert g.get_param("LoggingStorage") == v
    with pytest.raises(KeyError):
        g.set_param("LoggingStorage", 5)
    g.close()


# ---- 2. the replay kernel at its awkward shapes (seam level) -------------------------------------------------------------
EDGE_COUNTS = [0, 1, 63, 64, 65, 257, 0, 1000]
PLANE_COUNTS = [1000, 0, 257, 65, 1, 64, 63, 0]  # the last frame's planes are empty


@pytest.fixture(scope="module")
def seam_case(L):
    rng = np.random.default_rng(20261017)

    def cloud(n):
        p = np.zeros(n, L.POINT_DTYPE)
        for c in "xyz":
            p[c] = rng.uniform(-60, 60, n).astype(np.float32)
        p["w"] = 1.0
        p["time"] = rng.uniform(-0.1, 0.0, n)
        p["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
        p["laser_id"] = rng.integers(0, 16, n)
        return p

    log = [[cloud(e), cloud(p), cloud(0)] for e, p in zip(EDGE_COUNTS, PLANE_COUNTS)]
    P = [np.eye(4)]
    P[0][:3, :3] = rot(rng.normal(size=3), 0.3)
    P[0][:3, 3] = rng.uniform(-5, 5, 3)
    for _ in range(len(log) - 1):
        D = np.eye(4)
        D[:3, :3] = rot(rng.normal(size=3), rng.uniform(0.05, 0.3))  # up to 0.3 rad between neighbours
        D[:3, 3] = rng.uniform(-1, 1, 3)
        P.append(P[-1] @ D)
    t = 100.0 + 0.1 * np.arange(len(log)) + rng.uniform(0, 0.01, len(log))
    return log, np.array(P), t


def check_replay(L, O, ctx, log, P, t, undistort):
    outs, mn, mx = ctx.kplog_replay(P, t, undistort=undistort)
    for k in range(3):
        exp = expected_replay(O, [fr[k] for fr in log], P, t, undistort)
        whole = np.concatenate(exp) if exp else np.zeros(0, L.POINT_DTYPE)
        assert outs[k].size == whole.size
        assert outs[k].tobytes() == whole.tobytes(), (k, undistort)
        lo, hi = box_of(exp[-1])
        assert mn[k].tobytes() == lo.tobytes() and mx[k].tobytes() == hi.tobytes(), (k, mn[k], lo, mx[k], hi)


@pytest.mark.parametrize("chunk_kib", [-1, 48])
@pytest.mark.parametrize("undistort", [1, 0])
def test_replay_at_awkward_shapes(L, O, gpu_ctx, seam_case, undistort, chunk_kib):
    log, P, t = seam_case
    ctx = gpu_ctx
    ctx.kplog_clear()
    ctx.debug_set("kplog_chunk_kib", chunk_kib)  # 48 KiB: the eight frames take several chunks
    try:
        for fr in log:
            ctx.kplog_append_points(fr)
        assert ctx.kplog_size() == len(log)
        assert [ctx.kplog_count(i, 0) for i in range(len(log))] == EDGE_COUNTS
        assert [ctx.kplog_count(i, 1) for i in range(len(log))] == PLANE_COUNTS
        assert ctx.kplog_get(5, 0).tobytes() == log[5][0].tobytes()
        held = ctx.kplog_bytes()
        assert held >= sum(a.nbytes for fr in log for a in fr)
        if chunk_kib > 0:
            assert held % (chunk_kib << 10) == 0 and held > (chunk_kib << 10)
        check_replay(L, O, ctx, log, P, t, undistort)
        # the oldest frame dropped: the remaining seven under their own poses
        ctx.kplog_pop_front()
        assert ctx.kplog_size() == len(log) - 1 and ctx.kplog_get(0, 0).tobytes() == log[1][0].tobytes()
        check_replay(L, O, ctx, log[1:], P[1:], t[1:], undistort)
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_replay(P, t, undistort=undistort)  # eight poses for seven frames
        assert e.value.code == L.E_ARG
        # a log of exactly two frames
        for _ in range(len(log) - 3):
            ctx.kplog_pop_front()
        check_replay(L, O, ctx, log[-2:], P[-2:], t[-2:], undistort)
        ctx.kplog_pop_front()
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_replay(P[-1:], t[-1:], undistort=undistort)
        assert e.value.code == L.E_ARG
        # popped chunks are reused: a frame appended now needs no new memory
        ctx.kplog_append_points(log[0])
        assert ctx.kplog_bytes() == held
    finally:
        ctx.kplog_clear()
        ctx.debug_set("kplog_chunk_kib", -1)
    assert ctx.kplog_size() == 0 and ctx.kplog_bytes() == 0


def test_a_chunk_that_cannot_be_allocated_stops_the_log(L, gpu_ctx, seam_case):
    log, P, t = seam_case
    ctx = gpu_ctx
    ctx.kplog_clear()
    try:
        ctx.debug_set("kplog_fail_alloc", 1)
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_append_points(log[0])
        assert e.value.code == L.E_HIP and "could not be allocated" in str(e.value)
        assert ctx.kplog_stopped() and ctx.kplog_size() == 0
        ctx.debug_set("kplog_fail_alloc", 0)
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_append_points(log[0])  # stopped until the log is cleared
        assert e.value.code == L.E_STATE
        ctx.kplog_clear()
        assert not ctx.kplog_stopped()
        ctx.kplog_append_points(log[0])
        assert ctx.kplog_size() == 1
    finally:
        ctx.debug_set("kplog_fail_alloc", 0)
        ctx.kplog_clear()


# ---- 3. the rebuilt maps are the reference's rebuilt maps ---------------------------------------------------------------
def bend(P):
    """P'[i] = C[i] P[i]: a yaw of 0.002 i rad and a translation of 0.05 i m"""
    out = []
    for i, Pi in enumerate(P):
        C = np.eye(4)
        C[:3, :3] = rot([0, 0, 1], 0.002 * i)
        C[:3, 3] = 0.05 * i * np.array([0.6, 0.8, 0.0])
        out.append(C @ Pi)
    return np.array(out)


def mapped(L, frames, n=NFRAMES, **params):
    s = L.Slam(0, **{**dict(EgoMotion=3, LoggingTimeout=-1), **params})
    for f in range(n):
        s.add_frame(frames[f][0], frames[f][1], f)
    return s


def expected_maps(L, O, s, raw, P2, t, undistort, types):
    """per type the map the reference is left with (Slam.cxx:462-477), from a fresh oracle grid with the Slam's parameters"""
    maps = {}
    for k in types:
        exp = expected_replay(O, [raw[i][k] for i in range(len(P2))], P2, t, undistort)
        agg = np.concatenate(exp)
        params = dict(VoxelResolution=s.get_param("VoxelGridResolution"), GridSize=s.get_param("VoxelGridSize"), LeafSize=LEAVES[k],
                      Sampling=s.get_param("VoxelGridSamplingMode"), MinFramesPerVoxel=s.get_param("VoxelGridMinFramesPerVoxel"),
                      DecayingThreshold=s.get_param("VoxelGridDecayingThreshold"))
        grid = O.RollingGrid(**params)
        grid.add(agg, fixed=False, time=-1.0, roll=False)
        if agg.size:
            # the condition of this test, on the oracle's side: the grid as it stands (not rolled) holds the aggregate --
            # at least 90 % of the voxels a grid eight times as wide would hold
            wide = O.RollingGrid(**{**params, "GridSize": 8 * params["GridSize"]})
            wide.add(agg, fixed=False, time=-1.0, roll=False)
            assert wide.size() > 100 and grid.size() >= 0.9 * wide.size(), (k, grid.size(), wide.size())
        lo, hi = box_of(exp[-1])
        grid.roll(lo, hi)
        maps[k] = grid.get()
    return maps


@pytest.mark.parametrize("undistortion,on_device,sampling,blobs", [
    (2, 1, None, 0), (0, 1, None, 0), (2, 0, None, 0), (0, 0, None, 0), (2, 1, 4, 0), (2, 0, 4, 0), (2, 1, None, 1)])
def test_rebuilt_maps_are_the_references(L, O, frames, raw_keypoints, undistortion, on_device, sampling, blobs):
    params = dict(Undistortion=undistortion, MapsOnDevice=on_device, UseBlobs=blobs)
    if sampling is not None:
        params["VoxelGridSamplingMode"] = sampling
    s = mapped(L, frames, **params)
    types = types_in_use(L, blobs)
    P, t, cov = s.trajectory()
    assert P.shape[0] == NFRAMES == s.logged_frames()
    for k in types:  # the log holds what the expectation is built from
        assert s.logged_keypoints(3, k).tobytes() == raw_keypoints[3][k].tobytes()
    P2 = bend(P)
    want = expected_maps(L, O, s, raw_keypoints, P2, t, undistortion != 0, types)
    s.set_trajectory(P2, t)
    for k in types:
        got = s.map(k)
        assert got.size == want[k].size and got.size > 100, (k, got.size, want[k].size)
        assert got.tobytes() == want[k].tobytes(), k
    assert s.world_transform().tobytes() == P2[-1].tobytes()
    Pn, tn, covn = s.trajectory()
    assert Pn.tobytes() == P2.tobytes() and tn.tobytes() == t.tobytes()
    assert covn.tobytes() == cov.tobytes()  # the covariance log is kept
    assert s.logged_frames() == NFRAMES
    s.close()


# ---- 4. refusals leave everything alone ----------------------------------------------------------------------------------
def snapshot(L, s, types=(0, 1)):
    P, t, cov = s.trajectory()
    logged = [s.logged_keypoints(i, k).tobytes() for i in range(s.logged_frames()) for k in types]
    return [s.map(k).tobytes() for k in types], s.world_transform().tobytes(), P.tobytes(), t.tobytes(), cov.tobytes(), logged, s.get_param("NbrFrameProcessed")


def test_refusals_leave_everything_alone(L, frames):
    s = mapped(L, frames)
    P, t, _ = s.trajectory()
    P2 = bend(P)
    before = snapshot(L, s)
    off = t.copy()
    off[4] += 1e-3
    for poses, times, code in [(P2[:-1], t[:-1], L.E_ARG), (P2[:1], t[:1], L.E_ARG), (P2, off, L.E_ARG)]:
        with pytest.raises(L.LsaError) as e:
            s.set_trajectory(poses, times)
        assert e.value.code == code, (e.value, code)
        assert snapshot(L, s) == before
    s.close()
    q = mapped(L, frames, n=3, LoggingTimeout=0)
    Pq, tq, _ = q.trajectory()
    assert Pq.shape[0] == 2 and q.logged_frames() == 0
    before = snapshot(L, q)
    with pytest.raises(L.LsaError) as e:
        q.set_trajectory(bend(Pq), tq)
    assert e.value.code == L.E_STATE
    assert snapshot(L, q) == before
    q.close()


def test_a_failed_chunk_stops_logging_and_not_the_frames(L, frames):
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    s.context().debug_set("kplog_fail_alloc", 1)  # the log's first chunk cannot be had
    s.add_frame(frames[0][0], frames[0][1], 0)  # goes on
    assert "keypoint logging stopped" in s.L.lsa_slam_last_error(s.h).decode()
    s.context().debug_set("kplog_fail_alloc", 0)
    for f in (1, 2):
        s.add_frame(frames[f][0], frames[f][1], f)
    assert s.get_param("NbrFrameProcessed") == 3 and s.trajectory()[1].size == 3 and s.logged_frames() == 0
    P, t, _ = s.trajectory()
    with pytest.raises(L.LsaError) as e:
        s.set_trajectory(P, t)
    assert e.value.code == L.E_STATE
    s.reset(True)  # logging starts again
    for f in range(2):
        s.add_frame(frames[f][0], frames[f][1], f)
    assert s.logged_frames() == 2
    P, t, _ = s.trajectory()
    s.set_trajectory(P, t)
    s.close()


# ---- 5. life goes on -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [1, 0])
def test_life_goes_on_after_a_rebuild(L, frames, on_device):
    s = mapped(L, frames, MapsOnDevice=on_device)
    P, t, _ = s.trajectory()
    P2 = bend(P)
    s.set_trajectory(P2, t)
    done = s.get_param("NbrFrameProcessed")
    for f in (NFRAMES, NFRAMES + 1):
        s.add_frame(frames[f][0], frames[f][1], f)
    assert s.get_param("NbrFrameProcessed") == done + 2
    Pn, tn, _ = s.trajectory()
    assert Pn.shape[0] == NFRAMES + 2 == s.logged_frames()
    assert Pn[:NFRAMES].tobytes() == P2.tobytes()
    assert np.all(np.isfinite(Pn)) and np.all(np.isfinite(s.world_transform()))
    assert s.get_param("DeviceSolveFallbacks") == 0
    # the two frames were registered in the rebuilt map: they go on from the bent trajectory's end at the sensor's speed
    step = np.linalg.norm(Pn[-1][:3, 3] - Pn[-2][:3, 3])
    assert 0.1 < step < 1.0 and np.linalg.norm(Pn[NFRAMES][:3, 3] - P2[-1][:3, 3]) < 1.0
    s.close()
