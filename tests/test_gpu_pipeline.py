"""GPU parity, seam 4 (undistortion / transforms) and the whole AddFrame pipeline against the CPU
oracle.  Bar: float outputs of the transforms bit-exact (double math, one rounding to float, same
operation order); keypoint sets bit-exact; poses within the north-star tolerance 1e-4 m / 1e-4 rad
measured with the reference's own regression protocol (LidarSlamTestNode.cxx:297-305) -- in practice
they agree to ~1e-12, the test keeps 1e-7 so that a real regression cannot hide."""
import time

import numpy as np
import pytest

from conftest import pose_diff, two_device_rig

pytestmark = pytest.mark.gpu


def se3(dx, dy, dz, rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    T = np.eye(4)
    T[:3, :3] = [[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz], [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz], [-sy, sx * cy, cx * cy]]
    T[:3, 3] = [dx, dy, dz]
    return T


@pytest.fixture(scope="module")
def scan(L):
    return L.synth_frame(16, 1000, 2)[0]


def test_undistortion_bit_exact(gpu_ctx, O, L, scan):
    """Slam::RefineUndistortion: per-point slerp between two poses (MotionModel.h:115-129)"""
    H0 = se3(0.01, -0.02, 0.0, 0.001, 0.0, -0.003)
    H1 = se3(0.52, 0.03, -0.01, -0.004, 0.002, 0.021)
    kp = [scan[::7], scan[3::11], scan[::3]]
    for case, (A, B, t0, t1) in {
        "generic": (H0, H1, -0.1, 0.0),
        "large rotation": (se3(0, 0, 0, 0.3, -0.2, 1.0), se3(1, 2, 3, -0.5, 0.4, -2.0), -0.1, 0.0),
        "t0 == t1: invalid interpolator, H0 applied": (H0, H1, 0.0, 0.0),
        "H0 == H1": (H1, H1, -0.1, 0.0),
        "identity": (np.eye(4), np.eye(4), -0.1, 0.0),
        "extrapolation outside [t0, t1]": (H0, H1, -0.05, -0.02),
    }.items():
        for k in range(3):
            gpu_ctx.set_keypoints(L.SET_RAW_CURRENT, k, kp[k])
        gpu_ctx.reset_working_keypoints()
        gpu_ctx.undistort(A, B, t0, t1)
        for k in range(3):
            assert gpu_ctx.keypoints(L.SET_WORKING, k).tobytes() == O.undistort(kp[k], A, B, t0, t1).tobytes(), (case, k)
            assert gpu_ctx.keypoints(L.SET_RAW_CURRENT, k).tobytes() == kp[k].tobytes()  # raw keypoints untouched
        # lsa_localization_begin: the same reset + undistortion, and the boxes under the pose guess, in one launch
        Tw = se3(12.5, -3.25, 0.75, 0.02, -0.01, 0.6)
        boxes = gpu_ctx.keypoint_bboxes(L.SET_WORKING, Tw)
        for arm in (True, False):  # the words armed ahead (between two frames), or by the call itself
            gpu_ctx.localization_begin(A, B, t0, t1, box_pose=Tw, arm=arm)
            for k in range(3):
                assert gpu_ctx.keypoints(L.SET_WORKING, k).tobytes() == O.undistort(kp[k], A, B, t0, t1).tobytes(), (case, k)
            got = gpu_ctx.keypoint_bboxes_end()
            assert got[0].tobytes() == boxes[0].tobytes() and got[1].tobytes() == boxes[1].tobytes(), case
        gpu_ctx.localization_begin(box_pose=Tw)  # no undistortion: working = raw
        plain = gpu_ctx.keypoint_bboxes_end()
        for k in range(3):
            assert gpu_ctx.keypoints(L.SET_WORKING, k).tobytes() == kp[k].tobytes()
        want = gpu_ctx.keypoint_bboxes(L.SET_RAW_CURRENT, Tw)
        assert plain[0].tobytes() == want[0].tobytes() and plain[1].tobytes() == want[1].tobytes()
        gpu_ctx.localization_begin(A, B, t0, t1)  # no boxes
        assert gpu_ctx.keypoints(L.SET_WORKING, 0).tobytes() == O.undistort(kp[0], A, B, t0, t1).tobytes()
    tr = gpu_ctx.working_time_range()
    allk = np.concatenate(kp)
    assert tr == (allk["time"].min(), allk["time"].max())


def test_rigid_transforms_bit_exact(gpu_ctx, O, L, scan):
    T = se3(12.5, -3.25, 0.75, 0.02, -0.01, 0.6)
    kp = scan[::5]
    gpu_ctx.set_keypoints(L.SET_WORKING, 1, kp)
    ref = O.transform(kp, T)
    assert gpu_ctx.transformed_keypoints(L.SET_WORKING, 1, T).tobytes() == ref.tobytes()  # Slam::TransformPointCloud
    mn, mx = gpu_ctx.working_bbox(1, T)  # getMinMax3D of the world keypoints (Slam.cxx:1026-1029)
    assert mn.tolist() == [ref["x"].min(), ref["y"].min(), ref["z"].min()] and mx.tolist() == [ref["x"].max(), ref["y"].max(), ref["z"].max()]
    gpu_ctx.set_keypoints(L.SET_RAW_CURRENT, 1, kp)
    gpu_ctx.transform_keypoints(L.SET_RAW_CURRENT, 1, T, 0.25)  # AggregateFrames(..., false): LIDAR -> BASE + time offset
    out = gpu_ctx.keypoints(L.SET_RAW_CURRENT, 1)
    exp = ref.copy()
    exp["time"] += 0.25
    assert out.tobytes() == exp.tobytes()


def test_registered_frame_bit_exact(gpu_ctx, O, L, scan):
    """Slam::AggregateFrames(frames, true): the whole scan to WORLD, rigid and interpolated"""
    gpu_ctx.upload_frame(scan)
    T = se3(3.0, 0.1, 0.0, 0.0, 0.01, 0.1)
    assert gpu_ctx.transform_frame(T).tobytes() == O.transform(scan, T).tobytes()
    H0, H1 = se3(2.5, 0.08, 0.0, 0.0, 0.009, 0.09), T
    assert gpu_ctx.transform_frame(H0, H1, -0.1, 0.0).tobytes() == O.undistort(scan, H0, H1, -0.1, 0.0).tobytes()


# ---------------------------------------------------------------------------------------- pipeline
def run_both(L, O, model, nframes, seed=1000, check_keypoints=True, **params):
    params.setdefault("EgoMotion", 3)
    oracle_params = {k: v for k, v in params.items() if k != "MapsOnDevice"}  # where the maps live is ours alone
    sg, so = L.Slam(0, **params), O.Slam(**oracle_params)
    worst = (0.0, 0.0)
    poses = []
    for f in range(nframes):
        pts, stamp = L.synth_frame(model, seed, f)
        sg.add_frame(pts, stamp, f)
        so.add_frame(pts, stamp, f)
        Tg, To = sg.world_transform(), so.world_transform()
        dp, da = pose_diff(To, Tg)
        worst = (max(worst[0], dp), max(worst[1], da))
        assert dp < 1e-4 and da < 1e-4, f"frame {f}: north-star tolerance exceeded ({dp} m, {da} rad)"
        assert dp < 1e-7 and da < 1e-6, f"frame {f}: poses drift apart ({dp} m, {da} rad; solves redone on the host: {sg.get_param('DeviceSolveFallbacks')})"
        if check_keypoints:
            for k in range(3):
                assert sg.keypoints(k, which=2).tobytes() == so.keypoints(k, which=2).tobytes(), f"frame {f}: raw keypoints {k}"
        poses.append(Tg)
    return sg, so, np.array(poses), worst


def test_pipeline_pose_parity_vlp16(L, O):
    """BASELINE.json config 2: VLP-16, extraction + ego-motion ICP + localization"""
    sg, so, poses, worst = run_both(L, O, 16, 12)
    st = sg.stats()
    assert st[12] > 1000 and st[9] >= 1 and st[10] >= 1  # matched keypoints, both ICP loops ran
    # undistorted and world keypoints of the last frame
    for k in range(2):
        a, b = sg.keypoints(k, which=0), so.keypoints(k, which=0)
        assert a.size == b.size
        d = np.abs(np.stack([a["x"] - b["x"], a["y"] - b["y"], a["z"] - b["z"]])).max()
        assert d < 1e-5  # float coordinates after the same chain of pose-dependent transforms
    assert np.abs(sg.covariance() - so.covariance()).max() <= 1e-6 * np.abs(so.covariance()).max()
    sg.close()


def test_pipeline_pose_parity_hdl64(L, O):
    """BASELINE.json config 3: HDL-64, full ego-motion + localization against the rolling map"""
    sg, _, _, _ = run_both(L, O, 64, 5)
    sg.close()


def test_pipeline_pose_parity_vls128(L, O):
    """BASELINE.json config 4 at full size (~260k points per scan)"""
    sg, _, _, _ = run_both(L, O, 128, 4)
    sg.close()


@pytest.mark.parametrize(
    "params",
    [
        dict(EgoMotion=1),  # library default: extrapolation only
        dict(EgoMotion=0),
        dict(EgoMotion=2, Undistortion=0),
        dict(EgoMotion=3, Undistortion=1),
        dict(EgoMotion=3, UseBlobs=1),
        dict(EgoMotion=3, TwoDMode=1),
        dict(EgoMotion=3, EgoMotionICPMaxIter=2, LocalizationICPMaxIter=2, LocalizationLMMaxIter=5),
        dict(EgoMotion=3, VoxelGridLeafSizeEdges=0.2, VoxelGridLeafSizePlanes=0.3, LocalizationEdgeNbNeighbors=9, LocalizationPlaneNbNeighbors=7,
             LocalizationMaxNeighborsDistance=3.0),  # indoor yaml of the reference
    ],
)
def test_pipeline_modes(L, O, params):
    sg, _, _, _ = run_both(L, O, 8, 6, **params)
    sg.close()


@pytest.mark.parametrize(
    "params",
    [
        dict(),                                                             # every frame a keyframe after the ramp-up
        dict(KfDistanceThreshold=1.2),                                      # sub-maps reused between keyframes
        dict(VoxelGridDecayingThreshold=0.45, VoxelGridMinFramesPerVoxel=2),  # ClearOldPoints + filtered sub-maps
        dict(VoxelGridSamplingMode=1), dict(VoxelGridSamplingMode=3), dict(VoxelGridSamplingMode=4),  # LAST, CENTER_POINT, CENTROID
        dict(MapUpdate=0),                                                  # no map: localization has nothing to match
    ],
)
@pytest.mark.parametrize("on_device", [1, 0])
def test_map_maintenance_beside_the_device_work(L, O, params, on_device):
    """30 frames against the oracle's maps.  Maps on the device (the default): keyframes are keyed, sorted, folded and
    merged into the sorted voxel arrays by kernels, the sub-maps are compacted straight into the kNN target.  Maps on
    the host ("MapsOnDevice" = 0): the insertions run on worker threads beside the next
    frame, the sub-maps are extracted ahead of time under the predicted pose.  Either way the trajectory must not
    know (same maps, same sub-map order), and map and sub-map are the oracle's, byte for byte."""
    sg, so, poses, _ = run_both(L, O, 8, 30, check_keypoints=False, MapsOnDevice=on_device, **params)
    assert sg.get_param("DeviceMapsInUse") == (1.0 if on_device else 0.0)  # every sampling mode, CENTROID too (round 3)
    if params.get("MapUpdate", 2) != 0:
        # sub-maps extracted ahead of time for the predicted boxes were kept (host maps: by the map workers; device maps:
        # on the look-ahead stream -- not for decaying maps, whose ClearOldPoints comes first in the localization)
        decaying_on_device = on_device and "VoxelGridDecayingThreshold" in params
        assert (sg.get_param("SubMapSpeculationHits") > 0) == (not decaying_on_device)
    for k in range(3):
        assert sg.map(k).tobytes() == so.map(k).tobytes()
        assert sg.map(k, clean=True).tobytes() == so.map(k, clean=True).tobytes()
        assert sg.target_submap(k).tobytes() == so.submap(k).tobytes()
    step = np.linalg.norm(poses[-1][:3, 3] - poses[10][:3, 3])
    assert step > 5.0 or params.get("MapUpdate", 2) == 0  # it moved: 5 m/s for 2 s
    sg.close()


@pytest.mark.parametrize("replay", [False, True])
def test_degenerate_frames_in_the_middle_of_a_sequence(L, O, replay):
    """frames that give too few keypoints, or none: "Not enough keypoints ... skipped for this frame" on both sides
    (Slam.cxx:919-923, 1098-1107), the pose is kept, the next good frame carries on -- with the map workers and the
    ahead-of-time sub-maps in between.  (Non-finite coordinates are not part of this: the reference builds kd-trees
    on them and queries with them, which is undefined there; here such keypoints simply find no neighbours.)"""
    sg, so = L.Slam(0, EgoMotion=3), O.Slam(EgoMotion=3)
    rng = np.random.default_rng(5)
    scans = []
    for f in range(14):
        pts, stamp = L.synth_frame(8, 1000, f)
        if f in (4, 9):
            pts = pts[pts["laser_id"] == 3][:40].copy()          # one short ring: nothing can be extracted
        elif f in (6, 10):
            keep = rng.random(pts.size) < 0.02                   # 2 % of the points: a few keypoints at best
            pts = pts[keep].copy()
        scans.append((pts, stamp))
        if replay:
            sg.store_frame(f, pts)
    for f, (pts, stamp) in enumerate(scans):
        if replay:
            # from the frame store with the look-ahead: the extraction of the next (possibly degenerate) frame,
            # the ego-motion targets and the sub-maps are all prepared ahead of time
            if f + 1 < len(scans):
                sg.hint_next_stored_frame(f + 1)
            sg.add_stored_frame(f, stamp, f)
        else:
            sg.add_frame(pts, stamp, f)
        so.add_frame(pts, stamp, f)
        dp, da = pose_diff(so.world_transform(), sg.world_transform())
        assert dp < 1e-7 and da < 1e-6, (f, dp, da)
        for k in range(3):
            assert sg.keypoints(k, which=2).size == so.keypoints(k, which=2).size, (f, k)
    assert sg.world_transform()[0, 3] > 3.0
    sg.close()


def test_long_sequence_stays_on_the_oracle(L, O):
    """120 VLP-16 frames (12 s, 60 m): no drift between the two implementations, overlap estimate included"""
    sg, so = L.Slam(0, EgoMotion=3, OverlapSamplingRatio=0.25), O.Slam(EgoMotion=3, NbThreads=8, OverlapSamplingRatio=0.25)
    for f in range(120):
        pts, stamp = L.synth_frame(16, 1000, f)
        sg.add_frame(pts, stamp, f)
        so.add_frame(pts, stamp, f)
        dp, da = pose_diff(so.world_transform(), sg.world_transform())
        assert dp < 1e-9 and da < 1e-6, (f, dp, da)
    assert abs(sg.get_param("OverlapEstimation") - so.overlap()) < 1e-4
    assert 55.0 < sg.world_transform()[0, 3] < 65.0  # 5 m/s for 12 s
    sg.close()


def test_pipeline_matches_golden_poses(L, golden):
    s = L.Slam(0, EgoMotion=3)
    for f in range(4):
        s.add_frame(golden[f"frame{f}"], int(golden[f"stamp{f}"][0]), f)
        dp, da = pose_diff(golden["poses"][f], s.world_transform())
        assert dp < 1e-7 and da < 1e-6, (f, dp, da)
    s.close()


def test_pipeline_is_deterministic_and_resets(L):
    frames = [L.synth_frame(8, 1000, f) for f in range(4)]

    def run(s):
        out = []
        for f, (pts, stamp) in enumerate(frames):
            s.add_frame(pts, stamp, f)
            out.append(s.world_transform())
        return np.array(out)

    s = L.Slam(0, EgoMotion=3)
    a = run(s)
    s.reset()
    assert np.array_equal(s.world_transform(), np.eye(4))
    b = run(s)
    assert np.array_equal(a, b)  # bitwise: every reduction has a fixed order
    s.close()


def test_frame_checks_and_registered_frame(L, O):
    pts, stamp = L.synth_frame(8, 1000, 0)
    pts1, stamp1 = L.synth_frame(8, 1000, 1)
    sg, so = L.Slam(0, EgoMotion=3), O.Slam(EgoMotion=3)
    sg.add_frame(pts, 0, 0)  # stamp 0 == the post-reset previous stamp: frame dropped (Slam.cxx:727-731)
    assert np.array_equal(sg.world_transform(), np.eye(4)) and sg.stats()[0] == 0
    for s in (sg, so):
        s.add_frame(pts, stamp, 0)
        s.add_frame(pts1, stamp1, 1)
    T = sg.world_transform()
    sg.add_frame(pts1, stamp1, 2)  # same stamp: ignored
    assert np.array_equal(T, sg.world_transform())
    a, b = sg.registered_frame(), so.registered_frame()
    assert a.size == b.size == pts1.size
    assert np.abs(np.stack([a["x"] - b["x"], a["y"] - b["y"], a["z"] - b["z"]])).max() < 1e-5
    assert np.array_equal(a["time"], b["time"]) and np.array_equal(a["laser_id"], b["laser_id"])
    sg.close()


def test_match_debug_arrays_follow_the_oracle(L, O):
    """Slam::GetDebugArray 'EgoMotion/Localization: <type> matches' (Slam.cxx:635-657)"""
    sg, so = L.Slam(0, EgoMotion=3, KeepMatchDebug=1), O.Slam(EgoMotion=3)
    for f in range(3):
        pts, stamp = L.synth_frame(8, 1000, f)
        sg.add_frame(pts, stamp, f)
        so.add_frame(pts, stamp, f)
    total = same = 0
    for loc in (0, 1):
        for k in (0, 1):
            a, wa = sg.match_status(loc, k)
            b, wb = so.match_status(loc, k)
            assert a.size == b.size and a.size > 0
            total += a.size
            same += int((a == b).sum())
    # the poses of the two runs differ in the last bits (reduction order), so a keypoint sitting exactly
    # on a threshold may flip; everything else must agree
    assert same >= total - 2, (same, total)
    sg.close()


def test_stored_frames_equal_uploaded_frames(L):
    frames = [L.synth_frame(8, 1000, f) for f in range(3)]
    a, b = L.Slam(0, EgoMotion=3), L.Slam(0, EgoMotion=3)
    for f, (pts, stamp) in enumerate(frames):
        b.store_frame(f, pts)
    for f, (pts, stamp) in enumerate(frames):
        a.add_frame(pts, stamp, f)
        b.add_stored_frame(f, stamp, f)
        assert np.array_equal(a.world_transform(), b.world_transform())
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------- SURVEY.md 8f-3
def test_overlap_estimator_follows_the_oracle(gpu_ctx, O, L, scan):
    """Confidence::LCPEstimator (ConfidenceEstimators.cxx:27-65): nearest map point of every third frame point,
    best Gaussian score, mean.  The reference sums in float in no defined order: agreement to rounding."""
    ex = O.Extractor()
    ex.compute(scan)
    maps = [ex.keypoints(k) for k in range(3)]  # stand-ins for the three sub-maps
    gpu_ctx.upload_frame(scan)
    leaves = (0.3, 0.6, 0.3)
    H0, H1 = se3(0.05, 0.01, 0.0, 0.0, 0.001, 0.002), se3(0.3, 0.02, 0.0, 0.0, 0.002, 0.01)
    for k in range(3):
        gpu_ctx.set_target(k, maps[k], cell=1.0)
    # rigid and interpolated registration, all maps and a subset
    for mask, h1 in ((7, None), (3, H1), (2, H1)):
        tg = [maps[k] if (mask >> k) & 1 else None for k in range(3)]
        reg = O.transform(scan, H0) if h1 is None else O.undistort(scan, H0, h1, -0.1, 0.0)
        want = O.lcp(reg, 0.33, tg, leaves)
        got = gpu_ctx.overlap(mask, 0.33, leaves, H0, h1, -0.1, 0.0)
        assert 0.0 < want <= 1.0 and abs(got - want) <= 2e-5 * want, (mask, got, want)
    # nothing to estimate: no map, or no sampled point
    for k in range(3):
        gpu_ctx.set_target(k, maps[k][:0])
    assert gpu_ctx.overlap(7, 0.33, leaves, H0) == -1.0 == O.lcp(O.transform(scan, H0), 0.33, [None] * 3, leaves)
    gpu_ctx.set_target(1, maps[1])
    assert gpu_ctx.overlap(7, 1e-9, leaves, H0) == -1.0


def test_pipeline_overlap_estimation(L, O):
    """Slam::EstimateOverlap (Slam.cxx:1370-1388) inside AddFrame, with the ROS configuration's sampling ratio"""
    sg, so = L.Slam(0, EgoMotion=3, OverlapSamplingRatio=0.33), O.Slam(EgoMotion=3, OverlapSamplingRatio=0.33)
    seen = []
    for f in range(5):
        pts, stamp = L.synth_frame(16, 1000, f)
        sg.add_frame(pts, stamp, f)
        so.add_frame(pts, stamp, f)
        got, want = sg.get_param("OverlapEstimation"), so.overlap()
        assert (want == -1.0 and got == -1.0) or abs(got - want) <= 2e-5 * abs(want), (f, got, want)
        seen.append(want)
    assert seen[0] == -1.0 and all(0.3 < v <= 1.0 for v in seen[1:])  # no map before the first frame, then mostly overlapping


# ---------------------------------------------------------------------------------------- SURVEY.md 8f-4
VELODYNE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("pad2", "<u2"),
                     ("time", "<f4"), ("pad3", "<f4")])  # velodyne_pcl::PointXYZIRT, 32 bytes
VELODYNE_LAYOUT = (32, 0, 4, 8, 16, 20, 24)


def wire_records(pts, with_time=True):
    rec = np.zeros(pts.size, VELODYNE)
    for f in ("x", "y", "z", "intensity"):
        rec[f] = pts[f]
    rec["ring"] = pts["laser_id"]
    if with_time:
        rec["time"] = pts["time"].astype(np.float32)
    return rec


def same_points(a, b):
    """field by field (the identity transform used to read the frame back turns -0.0 into +0.0)"""
    return a.size == b.size and all(np.array_equal(a[f], b[f]) for f in a.dtype.names)


def test_wire_format_upload_follows_the_driver_node(O, L):
    """VelodyneToLidarNode::Callback (lidar_conversions/src/VelodyneToLidarNode.cxx:52-112) on the device: the frame the
    context holds after lsa_upload_wire_frame is the LidarPoint cloud the node would publish, value for value"""
    ctx = L.Context(0)
    eye = np.eye(4)
    mapping = np.arange(16, dtype=np.uint16)[::-1].copy()  # a custom laser id mapping: rings reversed
    try:
        for f, (mp, dev) in enumerate(((None, 0), (None, 3), (mapping, 1))):  # frame 0 goes through the host (resolution estimate)
            pts, _ = L.synth_frame(16, 1000, f)
            rec = wire_records(pts)
            want, valid = O.velodyne_to_lidar(rec, VELODYNE_LAYOUT, mp, dev)
            assert valid
            ctx.upload_wire_frame(rec, VELODYNE_LAYOUT, mp, dev)
            assert same_points(ctx.transform_frame(eye), want)
        # keypoints from the wire frame == keypoints from the converted cloud
        counts = ctx.extract_keypoints()
        ctx2 = L.Context(0)
        ctx2.azimuthal_resolution = ctx.azimuthal_resolution
        ctx2.upload_frame(want)
        assert counts.tolist() == ctx2.extract_keypoints().tolist()
        ctx2.close()
        # no usable time field: built from the azimuth advancement, first or last packet stamp
        pts, _ = L.synth_frame(16, 1000, 5)
        rec = wire_records(pts, with_time=False)
        for first in (False, True):
            want, valid = O.velodyne_to_lidar(rec, VELODYNE_LAYOUT, None, 0, 600.0, first)
            assert not valid and np.ptp(want["time"]) > 0.05
            # on the device: per ring "+ 1 behind a descent of the advancement, until a NaN resets the ring" on the ring-bucketed
            # frame; the arc tangent is the portable one, so the time agrees with the node's libm value to rounding
            ctx.upload_wire_frame(rec, VELODYNE_LAYOUT, None, 0, 600.0, first)
            got = ctx.transform_frame(eye)
            assert np.abs(got["time"] - want["time"]).max() < 2e-8 and np.ptp(got["time"]) > 0.05
            got["time"] = want["time"]
            assert same_points(got, want)
        # more than one turn in a frame, rings starting at different azimuths: the + 1 of the estimator comes into play
        rng = np.random.default_rng(3)
        n = 40000
        az = np.sort(rng.uniform(0.3, 0.3 + 2.3 * np.pi, n))  # 1.15 turns
        ring = rng.integers(0, 16, n)
        rr = rng.uniform(5, 30, n)
        spin = np.zeros(n, L.POINT_DTYPE)
        spin["x"], spin["y"], spin["z"], spin["w"] = rr * np.cos(-az), rr * np.sin(-az), 0.1 * ring, 1.0
        spin["laser_id"], spin["intensity"] = ring, 10.0
        rec = wire_records(spin, with_time=False)
        for first in (False, True):
            want, valid = O.velodyne_to_lidar(rec, VELODYNE_LAYOUT, None, 0, 600.0, first)
            ctx.upload_wire_frame(rec, VELODYNE_LAYOUT, None, 0, 600.0, first)
            got = ctx.transform_frame(eye)
            assert not valid and np.ptp(want["time"]) > 0.105 and np.abs(got["time"] - want["time"]).max() < 2e-8
    finally:
        ctx.close()


@pytest.mark.gpu
def test_sequences_side_by_side_on_one_gpu_reproduce_lone_runs():
    """Batch replay with several sequences per GPU (replay.ConcurrentReplay, bench.py --sequences-per-gpu): every
    sequence has its own handle and host thread, and nothing is shared between handles -- the poses of each one
    are those of a lone run, bit for bit, whatever the interleaving on the device."""
    from lidarslam_amd.replay import ConcurrentReplay

    frames = 10
    lone = []
    for seed in (1000, 1001, 1002, 1003):
        rep = ConcurrentReplay(0, 16, [seed], frames, EgoMotion=3)
        rep.run(2)
        lone.append(rep.poses[0].copy())
        rep.close()
    assert not np.array_equal(lone[0][-1], lone[1][-1])
    # eight sequences side by side, with the rolling maps on the host threads (what ConcurrentReplay picks for several
    # sequences) and on the device (what it picked for the lone runs above): the same poses, bit for bit
    seeds = [1000, 1001, 1002, 1003, 1000, 1001, 1002, 1003]
    for maps_on_device in (0, 1):
        rep = ConcurrentReplay(0, 16, seeds, frames, EgoMotion=3, MapsOnDevice=maps_on_device)
        fps = rep.run(2)
        assert fps > 0
        assert rep.slams[0].get_param("DeviceMapsInUse") == float(maps_on_device)
        for s, seed in enumerate(seeds):
            assert np.array_equal(rep.poses[s], lone[seed - 1000]), (maps_on_device, s)
        rep.close()
    with pytest.raises(ValueError):
        ConcurrentReplay(0, 16, [1000], 2, EgoMotion=3).run(2)


def _yaw_offset(deg, t):
    T = np.eye(4)
    a = np.deg2rad(deg)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


@pytest.mark.gpu
def test_result_getters_and_confidence_estimators_follow_the_oracle(L, O):
    """Slam.h:141-189 and :385-394 -- trajectory / covariance log with a timeout, latency-compensated pose, maps and
    target sub-maps, GetDebugInformation (matches used per type without reading anything back on the frame's critical
    path), motion limits, a BASE <- LIDAR offset and a pose guess in the middle of the sequence."""
    params = dict(EgoMotion=3, LoggingTimeout=0.45, TimeWindowDuration=0.25, VelocityLimitLinear=5.05, VelocityLimitAngular=400.0,
                  AccelerationLimitLinear=3.0, AccelerationLimitAngular=1e4, OverlapSamplingRatio=0.25)
    sg, so = L.Slam(0, **params), O.Slam(**params)
    offset = _yaw_offset(10.0, [0.5, -0.1, 1.0])
    sg.set_base_to_lidar_offset(offset), so.set_base_to_lidar_offset(offset)
    assert np.array_equal(sg.base_to_lidar_offset(), offset)
    with pytest.raises(L.LsaError):
        sg.set_base_to_lidar_offset(offset, device_id=300)  # device ids are 8 bits
    comply = []
    for f in range(14):
        pts, stamp = L.synth_frame(8, 1000, f)
        if f == 8:
            # a pose imposed from outside: the ego-motion is skipped for this frame on both sides
            guess = sg.world_transform() @ _yaw_offset(1.0, [0.3, 0.05, 0.0])
            sg.set_world_transform_from_guess(guess), so.set_world_transform_from_guess(guess)
        sg.add_frame(pts, stamp, f), so.add_frame(pts, stamp, f)
        Tg, To = sg.world_transform(), so.world_transform()
        assert np.abs(Tg - To).max() < 1e-9, f
        ig, io = sg.debug_information(), so.debug_information()
        for key in L.DEBUG_INFORMATION_NAMES[:5]:
            assert ig[key] == io[key], (f, key)
        for key in L.DEBUG_INFORMATION_NAMES[5:8]:
            assert abs(ig[key] - io[key]) <= 1e-6 * max(1.0, abs(io[key])), (f, key, ig[key], io[key])
        assert ig["Confidence: comply motion limits"] == io["Confidence: comply motion limits"], f
        comply.append(ig["Confidence: comply motion limits"])
        if f >= 2:
            assert ig["Localization: planes used"] > 20 and ig["Localization: edges used"] > 20
        # trajectory and covariance log: poses of the last 0.45 s (at least two)
        pg, tg, cg = sg.trajectory()
        po, to, co = so.trajectory()
        assert pg.shape == po.shape and np.array_equal(tg, to) and np.abs(pg - po).max() < 1e-9
        assert np.allclose(cg, co, rtol=1e-5, atol=1e-12)
        assert pg.shape[0] == min(f + 1, 5)
        # latency compensation: the reference measures the latency, the oracle is told the device path's
        so.set_param("Latency", sg.get_param("Latency"))
        assert np.abs(sg.latency_compensated_world_transform() - so.latency_compensated_world_transform()).max() < 1e-9
        for k in (L.EDGE, L.PLANE):
            assert sg.map(k).size == so.map(k).size and sg.map(k, clean=True).size == so.map(k, clean=True).size
            assert sg.target_submap(k).size == so.submap(k).size
    # 5 m/s against a 5.05 m/s limit: compliant while cruising, not across the imposed jump
    assert comply[7] == 1.0 and 0.0 in comply[8:11]
    sg.close()


@pytest.mark.gpu
def test_two_lidar_devices_follow_the_oracle(L, O):
    """Slam::AddFrames with one frame per LiDAR device: per-device extractor (own parameters and azimuthal
    resolution), BASE <- LIDAR offset and time shift, keypoints merged in frame order (bit-identical to the oracle),
    poses, registered frame of all devices and the overlap estimator on the aggregated cloud."""
    params = dict(EgoMotion=3, OverlapSamplingRatio=0.2)
    sg, so = L.Slam(0, **params), O.Slam(**params)
    for f in range(8):
        frames, stamps, offset = two_device_rig(L, f)
        if f == 0:
            for s in (sg, so):
                s.set_base_to_lidar_offset(offset, device_id=1)
                s.set_extractor_param(1, "EdgeIntensityGapThreshold", 40.0)
            assert sg.extractor_param(1, "EdgeIntensityGapThreshold") == 40.0 and sg.extractor_param(1, "NeighborWidth") == 4
            assert np.array_equal(sg.base_to_lidar_offset(1), offset) and np.array_equal(sg.base_to_lidar_offset(7), np.eye(4))
        if f == 5:
            frames[0] = frames[0][:0]  # the first device drops a frame: the pose is still dated by its stamp
        sg.add_frames(frames, stamps, f), so.add_frames(frames, stamps, f)
        for k in (L.EDGE, L.PLANE):
            kg, ko = sg.keypoints(k, 2), so.keypoints(k, 2)
            assert kg.size == ko.size and kg.tobytes() == ko.tobytes(), (f, k)
            if f != 5:
                assert set(np.unique(kg["device_id"])) == {0, 1}
        dt, dr = pose_diff(sg.world_transform(), so.world_transform())
        assert dt < 1e-9 and dr < 1e-9, (f, dt, dr)
        rg, ro = sg.registered_frame(), so.registered_frame()
        assert rg.size == ro.size == frames[0].size + frames[1].size
        for field in ("x", "y", "z"):
            assert np.abs(rg[field] - ro[field]).max() < 1e-4
        assert np.array_equal(rg["time"], ro["time"]) and np.array_equal(rg["device_id"], ro["device_id"])
        if f > 0:
            assert abs(sg.get_param("OverlapEstimation") - so.overlap()) < 1e-5, f
    # single frames of the second device take the same route (extractor and offset of that device)
    frames, stamps, offset = two_device_rig(L, 8)
    sg.add_frame(frames[1], stamps[1], 8), so.add_frame(frames[1], stamps[1], 8)
    kg, ko = sg.keypoints(L.PLANE, 2), so.keypoints(L.PLANE, 2)
    assert kg.size == ko.size > 0 and kg.tobytes() == ko.tobytes()
    dt, dr = pose_diff(sg.world_transform(), so.world_transform())
    assert dt < 1e-9 and dr < 1e-9
    sg.close()


@pytest.mark.gpu
def test_lookahead_extraction_changes_nothing_but_the_schedule(L):
    """lsa_slam_hint_next_stored_frame / lsa_extract_prefetch: the next stored frame's keypoints are extracted on their
    own stream beside the current frame's registration and adopted by the next AddStoredFrame.  Poses, keypoints and
    match statistics are those of the plain run bit for bit -- with hints that come true, with hints that do not, and
    when a parameter changes between the look-ahead and the frame."""
    frames = [L.synth_frame(16, 1000, f) for f in range(12)]

    def run(hints, change_at=None, ahead=1):
        s = L.Slam(0, EgoMotion=3, BuildTargetsAhead=ahead)
        for f, (pts, _) in enumerate(frames):
            s.store_frame(f, pts)
        poses, kps, used = [], [], []
        for f, (_, stamp) in enumerate(frames):
            if f == change_at:
                s.set_param("EdgeIntensityGapThreshold", 30.0)  # the look-ahead of this frame used 50: it is dropped
            if hints(f) is not None:
                s.hint_next_stored_frame(hints(f))
            s.add_stored_frame(f, stamp, f)
            poses.append(s.world_transform())
            kps.append([s.keypoints(k, 2).tobytes() for k in (L.EDGE, L.PLANE)])
            used.append(s.get_param("TotalMatchedKeypoints"))
        hits = s.get_param("LookaheadAdopted")
        built[ahead] = s.get_param("TargetsBuiltAheadAdopted")
        staged[ahead] = s.get_param("SubMapsStagedAheadAdopted")
        s.close()
        return np.array(poses), kps, used, hits

    built, staged = {}, {}
    plain = run(lambda f: None, ahead=0)
    # the ego-motion targets of the next frame built beside this frame's registration: two per frame from the second
    # frame on, same poses
    ahead_targets = run(lambda f: None, ahead=1)
    assert built == {0: 0, 1: 2 * (len(frames) - 1)}
    # ... and most of the sub-maps extracted for the predicted pose were on the device, grid built, before
    # Localization asked for them (how many depends on when the host threads finish: a schedule, not a result)
    assert staged[0] == 0 and 0 <= staged[1] <= 2 * len(frames)
    assert np.array_equal(plain[0], ahead_targets[0]) and plain[1] == ahead_targets[1] and plain[2] == ahead_targets[2]
    ahead = run(lambda f: f + 1 if f + 1 < len(frames) else None)
    wrong = run(lambda f: (f + 3) % len(frames))
    assert plain[3] == 0 and ahead[3] == len(frames) - 1 and wrong[3] == 0
    for other in (ahead, wrong):
        assert np.array_equal(plain[0], other[0]) and plain[1] == other[1] and plain[2] == other[2]
    plain_c = run(lambda f: None, change_at=6)
    ahead_c = run(lambda f: f + 1 if f + 1 < len(frames) else None, change_at=6)
    assert ahead_c[3] == len(frames) - 2  # all but the frame whose parameters changed under the look-ahead
    assert np.array_equal(plain_c[0], ahead_c[0]) and plain_c[1] == ahead_c[1]
    assert plain_c[1] != plain[1]
    # the hint of a slot that does not exist is reported, not fatal
    s = L.Slam(0, EgoMotion=3)
    s.store_frame(0, frames[0][0])
    s.hint_next_stored_frame(5)
    s.add_stored_frame(0, frames[0][1], 0)
    assert s.keypoints(L.PLANE, 2).tobytes() == plain[1][0][1]
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("two_d", [0, 1])
def test_one_launch_lm_and_host_driven_lm_agree(L, O, two_d):
    """DeviceLM: LocalOptimizer::Solve as one launch (lsa_solve_device) against one launch per evaluation
    (host/lsa_lm.cpp): the same trust-region decisions frame after frame (evaluations, ICP iterations, keyframes), poses
    equal to rounding, both on the oracle; the covariance comes from the normal equations the solve returns"""
    a, b, o = L.Slam(0, EgoMotion=3, DeviceLM=1, TwoDMode=two_d), L.Slam(0, EgoMotion=3, DeviceLM=0, TwoDMode=two_d), O.Slam(EgoMotion=3, TwoDMode=two_d)
    for f in range(10):
        pts, stamp = L.synth_frame(16, 1000, f)
        for s in (a, b, o):
            s.add_frame(pts, stamp, f)
        dp, da = pose_diff(b.world_transform(), a.world_transform())
        assert dp < 1e-9 and da < 1e-8, (f, dp, da)
        dp, da = pose_diff(o.world_transform(), a.world_transform())
        assert dp < 1e-7 and da < 1e-6, (f, dp, da)
        sa, sb = a.stats(), b.stats()
        assert sa[9:14].tolist() == sb[9:14].tolist(), (f, sa[9:14], sb[9:14])  # ICP iterations, LM evaluations, matches, keyframes
        ca, cb = a.covariance(), b.covariance()
        assert np.abs(ca - cb).max() <= 1e-8 * max(np.abs(cb).max(), 1e-30)
    assert a.context().solve_device_fallbacks() == 0
    a.close()
    b.close()


@pytest.mark.gpu
def test_host_frames_announced_ahead_change_nothing_but_the_schedule(L):
    """lsa_slam_hint_next_frame: the next HOST cloud is uploaded (pinned staging, copy stream, uploader thread) and its
    keypoints extracted beside the current frame's registration; AddFrame takes both over when it gets that very cloud.
    Poses, keypoints and match counts are those of the plain run bit for bit -- with hints that come true, with a hint
    for a cloud that is never added, and when the announced cloud is replaced by another one."""
    frames = [L.synth_frame(16, 1000, f) for f in range(12)]

    clouds = [L.Slam.cloud_pointer(pts) for pts, _ in frames]

    def run(hint, by_pointer=False):
        s = L.Slam(0, EgoMotion=3)
        poses, kps, used = [], [], []
        for f, (pts, stamp) in enumerate(frames):
            h = hint(f)
            if by_pointer:  # the calls bench.py makes: the clouds' pointers taken once, outside the loop
                if h is not None:
                    s.hint_next_frame_at(clouds[h])
                s.add_frame_at(clouds[f], stamp, f)
            else:
                if h is not None:
                    s.hint_next_frame(frames[h][0])
                s.add_frame(pts, stamp, f)
            poses.append(s.world_transform())
            kps.append([s.keypoints(k, 2).tobytes() for k in (L.EDGE, L.PLANE)])
            used.append(s.get_param("TotalMatchedKeypoints"))
        up, la = s.get_param("UploadsAdopted"), s.get_param("LookaheadAdopted")
        s.close()
        return np.array(poses), kps, used, up, la

    plain = run(lambda f: None)
    ahead = run(lambda f: f + 1 if f + 1 < len(frames) else None)
    wrong = run(lambda f: (f + 5) % len(frames))
    ahead_at = run(lambda f: f + 1 if f + 1 < len(frames) else None, by_pointer=True)
    assert ahead_at[3] == len(frames) - 1
    assert plain[3] == 0 and plain[4] == 0
    assert ahead[3] == len(frames) - 1  # every announced cloud was the one that came
    assert 1 <= ahead[4] <= len(frames) - 1  # the extraction ran ahead whenever the upload was enqueued in time
    assert wrong[3] == 0 and wrong[4] == 0
    for other in (ahead, wrong, ahead_at):
        assert np.array_equal(plain[0], other[0]) and plain[1] == other[1] and plain[2] == other[2]


@pytest.mark.gpu
def test_upload_ahead_through_the_c_abi(gpu_ctx, O, L):
    """lsa_upload_frame_begin / _ready / _adopt / lsa_extract_prefetch_uploaded: the frame uploaded ahead gives the
    keypoints of lsa_upload_frame + lsa_extract_keypoints; a frame that was not the announced one is not adopted"""
    import ctypes as C
    import time

    lib, h = L.lib(), gpu_ctx.h
    a, b = L.synth_frame(16, 1000, 0)[0], L.synth_frame(16, 1000, 1)[0]
    gpu_ctx.upload_frame(a)
    ref_a = gpu_ctx.extract_keypoints().copy()
    kp_a = [gpu_ctx.keypoints(L.SET_RAW_CURRENT, k).tobytes() for k in range(3)]
    gpu_ctx.upload_frame(b)
    ref_b = gpu_ctx.extract_keypoints().copy()
    kp_b = [gpu_ctx.keypoints(L.SET_RAW_CURRENT, k).tobytes() for k in range(3)]
    params = L.ExtractParams()
    assert lib.lsa_upload_frame_adopt(h, L.ptr(a), a.size) == 0  # nothing announced
    assert lib.lsa_upload_frame_begin(h, L.ptr(a), a.size) == 0
    t0 = time.time()
    while not lib.lsa_upload_frame_ready(h) and time.time() - t0 < 5:
        time.sleep(0.0005)
    assert lib.lsa_upload_frame_ready(h) == 1
    assert lib.lsa_extract_prefetch_uploaded(h, C.byref(params)) == 0
    assert lib.lsa_upload_frame_adopt(h, L.ptr(b), b.size) == 0  # another cloud than the announced one
    assert lib.lsa_upload_frame_adopt(h, L.ptr(a), a.size) == 1
    adopted0 = lib.lsa_extract_prefetch_adopted(h)
    counts = gpu_ctx.extract_keypoints()
    assert lib.lsa_extract_prefetch_adopted(h) == adopted0 + 1
    assert np.array_equal(counts, ref_a) and [gpu_ctx.keypoints(L.SET_RAW_CURRENT, k).tobytes() for k in range(3)] == kp_a
    # two clouds announced; the caller skips the first: it is given up cleanly, the second is adopted
    assert lib.lsa_upload_frame_begin(h, L.ptr(a), a.size) == 0
    assert lib.lsa_upload_frame_begin(h, L.ptr(b), b.size) == 0
    assert lib.lsa_upload_frame_adopt(h, L.ptr(b), b.size) == 1
    assert lib.lsa_upload_frame_adopt(h, L.ptr(a), a.size) == 0
    counts = gpu_ctx.extract_keypoints()
    assert np.array_equal(counts, ref_b) and [gpu_ctx.keypoints(L.SET_RAW_CURRENT, k).tobytes() for k in range(3)] == kp_b


@pytest.mark.gpu
def test_polydata_arrays_upload_follows_the_paraview_filter(O, L):
    """vtkSlam::PolyDataToPointCloud (vtkSlam.cxx:668-707) on the device, from the frame's own arrays (structure of
    arrays, several scalar types): the frame the context holds is the cloud the filter would build, value for value --
    stamp, relative times, mapped laser ids, null points dropped with the order kept -- and gives the same keypoints"""
    ctx = L.Context(0)
    eye = np.eye(4)
    try:
        for f, (xyz_t, time_t, lid_t, int_t, mapping, factor) in enumerate((
                (np.float32, np.float64, np.uint8, np.float32, None, 1.0),
                (np.float64, np.float64, np.uint16, np.uint8, np.arange(16, dtype=np.uint16)[::-1].copy(), 1e-6),
                (np.float32, np.float32, np.int32, np.float64, None, 1.0))):
            pts, stamp = L.synth_frame(16, 1000, f)
            xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(xyz_t)
            t = ((pts["time"] + stamp * 1e-6) / factor).astype(time_t)  # absolute lidar time in the filter's unit
            inten = pts["intensity"].astype(int_t)
            lid = pts["laser_id"].astype(lid_t)
            xyz[5::97] = 0  # null returns, as LidarView delivers them
            want, want_stamp, all_valid = O.polydata_to_point_cloud(xyz, t, lid, inten, mapping, factor)
            got_stamp, kept, ok = ctx.upload_polydata_frame(xyz, t, lid, inten, mapping, factor)
            assert (got_stamp, kept, ok) == (want_stamp, want.size, all_valid) and not ok
            assert same_points(ctx.transform_frame(eye), want)
        counts = ctx.extract_keypoints()
        ctx2 = L.Context(0)
        ctx2.azimuthal_resolution = ctx.azimuthal_resolution
        ctx2.upload_frame(want)
        assert counts.tolist() == ctx2.extract_keypoints().tolist() and counts[1] > 50
        ctx2.close()
        # nothing dropped: "allPointsAreValid"
        xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1)
        assert ctx.upload_polydata_frame(xyz, pts["time"], pts["laser_id"], pts["intensity"])[1:] == (pts.size, True)
    finally:
        ctx.close()


def test_the_maps_follow_a_setter_that_moves_them_between_device_and_host(L, O):
    """"MapsOnDevice" set in the middle of a sequence: the points change sides (as RollingGrid's own
    geometry setters put them back, counts start again) and the sequence goes on -- close to the trajectory that never
    switched, with the same number of map points right after the move"""
    ref = L.Slam(0, EgoMotion=3)
    sw = L.Slam(0, EgoMotion=3)
    for f in range(16):
        pts, stamp = L.synth_frame(8, 1000, f)
        if f == 6:
            before = [sw.map(k).size for k in range(3)]
            sw.set_param("MapsOnDevice", 0)
            assert sw.get_param("DeviceMapsInUse") == 0.0
            assert [sw.map(k).size for k in range(3)] == before and sum(before) > 500
        if f == 11:
            before = [sw.map(k).size for k in range(3)]
            sw.set_param("MapsOnDevice", 1)
            assert sw.get_param("DeviceMapsInUse") == 1.0
            assert [sw.map(k).size for k in range(3)] == before
        ref.add_frame(pts, stamp, f)
        sw.add_frame(pts, stamp, f)
        dp, da = pose_diff(ref.world_transform(), sw.world_transform())
        assert dp < 2e-2 and da < 2e-3, (f, dp, da)
    ref.close(), sw.close()


def test_sub_maps_ahead_of_time_change_nothing_but_the_schedule(L):
    """"SubMapsAhead": the sub-map for the predicted box, extracted on the device beside the ego-motion ICP and swapped in
    when the actual box touches the same outer voxels -- the same poses, maps and sub-maps, bit for bit, as extracting it
    when the localization asks"""
    # ("SubMapsAheadAdaptive" = 0: also where it comes late, as on this small sensor, where the pipeline gives it up by itself)
    a, b = L.Slam(0, EgoMotion=3, SubMapsAhead=1, SubMapsAheadAdaptive=0), L.Slam(0, EgoMotion=3, SubMapsAhead=0)
    for f in range(25):
        pts, stamp = L.synth_frame(16, 1000, f)
        for s in (a, b):
            s.add_frame(pts, stamp, f)
        assert np.array_equal(a.world_transform(), b.world_transform()), f
        for k in range(2):
            assert a.target_submap(k).tobytes() == b.target_submap(k).tobytes(), (f, k)
    for k in range(2):
        assert a.map(k).tobytes() == b.map(k).tobytes()
    assert a.get_param("SubMapSpeculationHits") > 20 and b.get_param("SubMapSpeculationHits") == 0
    a.close(), b.close()


@pytest.mark.gpu
def test_a_cloud_rewritten_after_it_was_announced_is_not_taken_over(L):
    """HintNextFrame identifies the announced cloud by address and size.  A buffer that is reused for another scan (a
    driver's ring buffer, an allocator handing the block out again) must not be answered with the copy made when it was
    announced: nothing announced survives Reset(), and a sample of the contents is compared when the cloud is adopted."""
    frames = [L.synth_frame(16, 1000, f) for f in range(4)]
    ref = L.Slam(0, EgoMotion=3)
    for f in (2, 3):
        ref.add_frame(frames[f][0], frames[f][1], f)
    want = ref.world_transform()
    want_kp = [ref.keypoints(k, 2).tobytes() for k in (L.EDGE, L.PLANE)]
    ref.close()

    # hint(A), reset, rewrite A in place, add_frame(A) must see the new contents
    s = L.Slam(0, EgoMotion=3)
    buf = frames[0][0].copy()
    s.add_frame(frames[1][0], frames[1][1], 0)
    s.hint_next_frame(buf)
    s.reset()
    for f in (2, 3):
        buf[:] = 0
        n = frames[f][0].size
        cloud = buf[:n] if n <= buf.size else frames[f][0].copy()
        cloud[:] = frames[f][0]
        s.add_frame(cloud, frames[f][1], f)
    assert np.array_equal(s.world_transform(), want)
    assert [s.keypoints(k, 2).tobytes() for k in (L.EDGE, L.PLANE)] == want_kp
    s.close()

    # the same without a reset in between: announced, rewritten in place (same address, same size), added
    s = L.Slam(0, EgoMotion=3)
    n = min(frames[2][0].size, frames[3][0].size)
    a, b = frames[2][0][:n].copy(), frames[3][0][:n].copy()
    plain = L.Slam(0, EgoMotion=3)
    plain.add_frame(a.copy(), frames[2][1], 0)
    plain.add_frame(b.copy(), frames[3][1], 1)
    buf = a.copy()
    s.hint_next_frame(buf)          # announces the contents of frame 2 ...
    s.add_frame(buf, frames[2][1], 0)  # ... which is the cloud that comes: taken over
    s.hint_next_frame(buf)          # announced again with the old contents,
    s.context().sync()
    time.sleep(0.05)                # (the uploader thread has copied it by now)
    buf[:] = b                      # rewritten in place,
    s.add_frame(buf, frames[3][1], 1)  # and added: the copy made when it was announced is stale
    assert np.array_equal(s.world_transform(), plain.world_transform())
    assert s.get_param("UploadsAdopted") == 1
    s.close()
    plain.close()


@pytest.mark.gpu
@pytest.mark.parametrize("model,nframes", [(16, 14), (64, 6)])
def test_icp_iterations_enqueued_ahead_change_nothing_but_the_schedule(L, model, nframes):
    """ICPAhead = 2 (the default): the whole ICP loop is enqueued at once and every solve leaves the pose, the start point and the undistortion of the iteration behind it on the device
    (lsa_icp_link: lsa_posemath.h's arithmetic on the device, the host repeats it on the same results).  Same launches,
    same inputs, same order: poses, match counts and match statuses are those of the loop that enqueues every iteration
    when its pose is known, bit for bit."""
    frames = [L.synth_frame(model, 1000, f) for f in range(nframes)]

    def run(**params):
        s = L.Slam(0, EgoMotion=3, **params)
        poses, used, status = [], [], []
        for f, (pts, stamp) in enumerate(frames):
            s.add_frame(pts, stamp, f)
            poses.append(s.world_transform())
            used.append(s.get_param("TotalMatchedKeypoints"))
            status.append([s.match_status(loc, k)[0].tobytes() for loc in (0, 1) for k in (L.EDGE, L.PLANE)])
        fb = s.get_param("DeviceSolveFallbacks")
        cov = s.covariance()
        s.close()
        return np.array(poses), used, status, cov, fb

    inline = run(ICPAhead=0)
    ahead = run(ICPAhead=2)
    assert ahead[4] == 0
    assert np.array_equal(inline[0], ahead[0]) and inline[1] == ahead[1] and inline[2] == ahead[2]
    assert np.array_equal(inline[3], ahead[3])
    # ... also without the refined undistortion (nothing rides in the search kernel), with a single LM iteration allowed, with
    # more iterations than one loop enqueues behind links (it falls back to the in-line loop), in 2D, with the maps on the host
    # and without any map update
    for extra in ({"Undistortion": 1}, {"Undistortion": 0}, {"LocalizationICPMaxIter": 1, "EgoMotionICPMaxIter": 2}, {"LocalizationICPMaxIter": 8, "EgoMotionICPMaxIter": 6},
                  {"TwoDMode": 1}, {"MapsOnDevice": 0}, {"UndistortInSearch": 0}):
        a = run(ICPAhead=0, **extra)
        b = run(ICPAhead=2, **extra)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2], extra
        assert b[4] == 0


@pytest.mark.gpu
def test_the_fall_backs_of_the_bounded_device_waits_are_exercised(L, O):
    """One wait on the device is bounded and has a fall-back on the host that a healthy run never takes: a workgroup of the
    one-launch solve that waits 20 ms for the others' sums abandons the exchange, all give up, the trust-region loop runs on
    the host (LSA_E_STATE, DeviceSolveFallbacks).  lsa_debug_set provokes it; the results must be those of the oracle."""
    frames = [L.synth_frame(16, 1000, f) for f in range(8)]

    def run(prepare=None, **params):
        s = L.Slam(0, EgoMotion=3, **params)
        poses = []
        for f, (pts, stamp) in enumerate(frames):
            if prepare:
                prepare(s, f)
            s.add_frame(pts, stamp, f)
            poses.append(s.world_transform())
        out = np.array(poses), s.get_param("DeviceSolveFallbacks")
        s.close()
        return out

    plain = run()
    assert plain[1] == 0
    # one solve of frames 2 and 5 is abandoned by its second workgroup (or by its only one)
    so = O.Slam(EgoMotion=3)
    ref = []
    for f, (pts, stamp) in enumerate(frames):
        so.add_frame(pts, stamp, f)
        ref.append(so.world_transform())
    # (with the loops enqueued whole -- ICPAhead = 2, the default -- the solve that gives up leaves "do not run" for the
    #  iterations behind it, the host redoes it and goes on in line; with nothing enqueued ahead)
    for block, mode in ((1, 2), (0, 2), (0, 0)):
        lm = run(lambda s, f: s.context().debug_set("lm_give_up_block", block) if f in (2, 5) else None, ICPAhead=mode)
        assert lm[1] == 2
        for f in range(len(frames)):
            dp, da = pose_diff(ref[f], lm[0][f])
            assert dp < 1e-7 and da < 1e-6, (block, f, dp, da)


@pytest.mark.gpu
def test_robosense_clouds_are_converted_as_the_driver_node_does(O, L):
    """RobosenseToLidarNode::Callback (lidar_conversions/src/RobosenseToLidarNode.cxx:58-125) on the device: the frame the
    context holds after lsa_upload_robosense_frame is the LidarPoint cloud the node would publish, byte for byte -- NaN
    records dropped, the second of two identical returns dropped (also across runs of NaN and across chunk borders of
    the kernels), RS16's own laser id mapping / a given mapping / none, the time from the position inside the ring."""
    ctx = L.Context(0)
    eye = np.eye(4)
    rng = np.random.default_rng(11)
    RS_DTYPE = np.dtype({"names": ["x", "y", "z", "intensity"], "formats": ["<f4"] * 4, "offsets": [0, 4, 8, 16], "itemsize": 32})  # pcl::PointXYZI
    RS_LAYOUT = (32, 0, 4, 8, 16)

    def organized(model, f, height, width, nan_share, dup_share):
        """a synthetic scan arranged as the driver publishes it: one row per laser, NaN where a ray gave nothing"""
        pts, _ = L.synth_frame(model, 1000, f)
        cloud = np.zeros((height, width), RS_DTYPE)
        for c in "xyz":
            cloud[c] = np.nan
        for r in range(height):
            row = pts[pts["laser_id"] == (r % model)][:width]
            for c in ("x", "y", "z", "intensity"):
                cloud[c][r, : row.size] = row[c]
        flat = cloud.reshape(-1)
        n = flat.size
        holes = rng.random(n) < nan_share
        flat["x"][holes] = np.nan
        runs = rng.integers(0, n - 3000, 3)
        for s in runs:
            flat["y"][s : s + 2500] = np.inf  # long runs without a return (they span the kernels' chunks of 1024)
        dup = np.nonzero(rng.random(n) < dup_share)[0]
        dup = dup[dup > 0]
        for c in "xyz":
            flat[c][dup] = flat[c][dup - 1]  # dual return mode: the second return equals the first
        return flat

    try:
        mapping = rng.permutation(40).astype(np.uint16)
        cases = [(16, 16, 1800, None, 0), (16, 16, 1800, None, 3), (16, 32, 1500, None, 0), (64, 40, 2048, mapping, 1), (16, 16, 1800, mapping[:16], 0)]
        for f, (model, height, width, mp, dev) in enumerate(cases):
            rec = organized(model, f, height, width, 0.05, 0.1)
            want = O.robosense_to_lidar(rec, width, height, RS_LAYOUT, mp, dev, 600.0)
            kept = ctx.upload_robosense_frame(rec, width, height, RS_LAYOUT, mp, dev, 600.0)
            assert kept == want.size and 0.5 * rec.size < kept < rec.size
            assert same_points(ctx.transform_frame(eye), want)
        # nothing but duplicates and NaN after the first point; a cloud without a single finite point
        rec = organized(16, 0, 16, 1800, 0.0, 0.0)
        for c in "xyz":
            rec[c][1:] = rec[c][0]
        rec["x"][5::7] = np.nan
        assert ctx.upload_robosense_frame(rec, 1800, 16, RS_LAYOUT) == 1 == O.robosense_to_lidar(rec, 1800, 16, RS_LAYOUT).size
        rec["z"][:] = np.nan
        assert ctx.upload_robosense_frame(rec, 1800, 16, RS_LAYOUT) == 0 == O.robosense_to_lidar(rec, 1800, 16, RS_LAYOUT).size
        # keypoints from the driver's cloud == keypoints from the converted cloud
        rec = organized(16, 1, 16, 1800, 0.02, 0.05)
        want = O.robosense_to_lidar(rec, 1800, 16, RS_LAYOUT)
        ctx.upload_robosense_frame(rec, 1800, 16, RS_LAYOUT)
        counts = ctx.extract_keypoints()
        ctx2 = L.Context(0)
        ctx2.azimuthal_resolution = ctx.azimuthal_resolution
        ctx2.upload_frame(want)
        assert counts.tolist() == ctx2.extract_keypoints().tolist() and counts[:2].min() > 100
        ctx2.close()
    finally:
        ctx.close()
