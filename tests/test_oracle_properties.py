"""Self-checks of the CPU oracle that need no reference: portable math vs libm,
kNN vs brute force, PCA / residual-record identities, LM behaviour, extractor invariants and edge
cases, recovery of the known synthetic motion."""
import numpy as np
import pytest

from conftest import pose_diff, two_device_rig


# ---------------------------------------------------------------- portable math
def ulp_err(a, ref):
    # 1 ulp of the result, but never finer than 1 ulp of 1.0: next to the zeros of sin / cos the
    # two-constant argument reduction is accurate in absolute, not in relative, terms
    ref = np.asarray(ref, np.float64)
    spacing = np.maximum(np.spacing(np.abs(ref)), np.finfo(np.float64).eps)
    return np.abs(a - ref) / spacing


def test_portable_trig_is_within_one_ulp_of_libm(O):
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-4, 4, 200000), rng.uniform(0, np.pi / 3, 100000), [0.0, 1e-300, np.pi / 4, -np.pi / 4, np.pi, 1e-9]])
    assert ulp_err(O.math(0, x), np.sin(x)).max() <= 1.0
    assert ulp_err(O.math(1, x), np.cos(x)).max() <= 1.0
    y, xx = rng.uniform(-10, 10, 200000), rng.uniform(-10, 10, 200000)
    assert ulp_err(O.math(2, xx, y), np.arctan2(y, xx)).max() <= 1.0
    # asin / acos (the pose algebra between two ICP iterations): the whole domain, both ends densely
    u = np.concatenate([rng.uniform(-1, 1, 200000), 1 - 10.0 ** rng.uniform(-17, 0, 20000), -1 + 10.0 ** rng.uniform(-17, 0, 20000), [1., -1., 0., 0.5, -0.5]])
    assert ulp_err(O.math(7, u), np.arcsin(u)).max() <= 1.0
    assert ulp_err(O.math(8, u), np.arccos(u)).max() <= 1.0
    assert np.isnan(O.math(7, np.array([1.5, -2.0, np.nan]))).all() and np.isnan(O.math(8, np.array([1.5, -2.0, np.nan]))).all()
    # the quadrant cases the analytic eigen-solver reaches: y >= 0
    assert O.math(2, np.array([1.0, 0.0, -1.0]), np.array([0.0, 1.0, 0.0])).tolist() == [0.0, np.pi / 2, np.pi]


# ---------------------------------------------------------------- kNN
@pytest.mark.parametrize("k", [1, 5, 8, 10, 16])
def test_kdtree_equals_brute_force(O, L, k):
    tgt, _ = L.synth_frame(8, 1000, 0)
    rng = np.random.default_rng(k)
    q = np.stack([tgt["x"], tgt["y"], tgt["z"]], 1)[rng.integers(0, tgt.size, 600)].astype(np.float64) + rng.normal(0, 0.3, (600, 3))
    q = np.concatenate([q, rng.uniform(-300, 300, (50, 3))])  # far outside the cloud too
    i1, d1, c1 = O.knn(tgt, q, k)
    i2, d2, c2 = O.knn(tgt, q, k, brute=True)
    assert np.array_equal(c1, c2) and np.array_equal(i1, i2) and np.array_equal(d1, d2)
    assert np.all(np.diff(d1, axis=1) >= 0)  # ascending


def test_knn_ties_are_broken_by_index(O, L):
    tgt = np.zeros(6, L.POINT_DTYPE)
    tgt["x"] = [1, -1, 1, -1, 2, 0]  # four points at the same distance from the origin
    tgt["w"] = 1
    idx, d2, cnt = O.knn(tgt, np.zeros((1, 3)), 4)
    assert idx[0].tolist() == [5, 0, 1, 2] and cnt[0] == 4
    idx, d2, cnt = O.knn(tgt[:3], np.zeros((1, 3)), 5)  # fewer points than k
    assert cnt[0] == 3


# ---------------------------------------------------------------- matcher records
def test_match_records_satisfy_model_identities(O, L, golden):
    pose = golden["match_pose"]
    st, w, rec, hist = O.match(golden["kp1_1"], golden["kp0_1"], 1, L.MatchParams.ego_motion(), pose)
    ok = st == 0
    assert ok.sum() > 50 and hist[0] == ok.sum() and hist.sum() == st.size
    A = rec[ok, :9].reshape(-1, 3, 3)
    # plane: A = n n^T is a symmetric rank-1 projector
    assert np.abs(A - A.transpose(0, 2, 1)).max() == 0
    assert np.abs(A @ A - A).max() < 1e-12
    assert np.abs(np.trace(A, axis1=1, axis2=2) - 1).max() < 1e-12
    assert np.all((w[ok] > 0) & (w[ok] <= 1)) and np.all(w[~ok] == 0) and np.all(rec[~ok] == 0)
    # X is the untransformed BASE point (KeypointsMatcher.cxx:185, 271)
    kp = golden["kp1_1"][ok]
    assert np.array_equal(rec[ok, 12:15], np.stack([kp["x"], kp["y"], kp["z"]], 1).astype(np.float64))
    st, w, rec, _ = O.match(golden["kp1_0"], golden["kp0_0"], 0, L.MatchParams.ego_motion(), pose)
    A = rec[st == 0, :9].reshape(-1, 3, 3)
    # line: A = I - n n^T projector of rank 2
    assert np.abs(A @ A - A).max() < 1e-12 and np.abs(np.trace(A, axis1=1, axis2=2) - 2).max() < 1e-12


def test_match_status_edge_cases(O, L, golden):
    cur, tgt = golden["kp1_1"], golden["kp0_1"]
    pose = np.eye(4)
    st, _, _, hist = O.match(cur, tgt[:0], 1, L.MatchParams.ego_motion(), pose)  # empty target
    assert np.all(st == 7) and hist.sum() == 0  # UNKOWN, histogram untouched (KeypointsMatcher.cxx:53-58)
    st, _, _, _ = O.match(cur, tgt[:3], 1, L.MatchParams.ego_motion(), pose)  # fewer points than k
    assert np.all(st == 2)  # NOT_ENOUGH_NEIGHBORS
    far = np.eye(4)
    far[0, 3] = 500.0
    st, _, _, _ = O.match(cur, tgt, 1, L.MatchParams.ego_motion(), far)
    assert np.all(st == 3)  # NEIGHBORS_TOO_FAR
    st, _, _, _ = O.match(cur, tgt, 1, L.MatchParams.ego_motion(plane_nb_neighbors=2), pose)
    assert np.all(st == 1)  # BAD_MODEL_PARAMETRIZATION
    st, _, _, _ = O.match(golden["kp1_0"], golden["kp0_0"], 0, L.MatchParams.ego_motion(edge_min_nb_neighbors=1), pose)
    assert np.all(st == 1)


# ---------------------------------------------------------------- LM
def make_plane_problem(n=400, seed=0):
    """Residual records of points on three orthogonal planes displaced by a known transform."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 16))
    normals = np.eye(3)[rng.integers(0, 3, n)]
    P = rng.uniform(-10, 10, (n, 3))
    w6 = np.array([0.3, -0.2, 0.1, 0.01, -0.02, 0.03])
    cx, sx, cy, sy, cz, sz = np.cos(w6[3]), np.sin(w6[3]), np.cos(w6[4]), np.sin(w6[4]), np.cos(w6[5]), np.sin(w6[5])
    R = np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz], [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz], [-sy, sx * cy, cx * cy]])
    X = (P - w6[:3]) @ R  # R^T (P - t): the true pose maps X back onto P
    rec[:, :9] = np.einsum("ni,nj->nij", normals, normals).reshape(n, 9)
    rec[:, 9:12] = P
    rec[:, 12:15] = X
    rec[:, 15] = 1.0
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, w6[:3]
    return rec, np.zeros(n, np.uint8), T


def test_lm_recovers_a_known_transform(O):
    rec, st, T = make_plane_problem()
    pose, w, summ, costs = O.lm_solve(rec, st, 5.0, np.eye(4), max_iter=15)
    dp, da = pose_diff(T, pose)
    assert dp < 1e-6 and da < 1e-6
    assert costs[1] < 1e-12 * max(costs[0], 1) + 1e-14 and summ[0] >= 2


def test_lm_reports_one_successful_step_at_the_optimum(O):
    rec, st, T = make_plane_problem()
    pose, w, summ, costs = O.lm_solve(rec, st, 5.0, T)
    assert summ[0] == 1  # "no LM step accepted": the ICP loops stop on this (Slam.cxx:950, 1151)
    assert pose_diff(T, pose)[0] < 1e-12


def test_lm_cost_never_increases_and_respects_max_iter(O):
    rec, st, T = make_plane_problem(seed=3)
    prev = None
    for it in range(0, 6):
        pose, w, summ, costs = O.lm_solve(rec, st, 5.0, np.eye(4), max_iter=it)
        assert summ[2] <= it and costs[1] <= costs[0]
        if prev is not None:
            assert costs[1] <= prev + 1e-12
        prev = costs[1]


def test_tukey_saturation_and_two_d_mode(O):
    rec, st, T = make_plane_problem()
    rec_out = rec.copy()
    rec_out[:40, 9:12] += 50.0  # gross outliers: beyond the saturation distance they carry no gradient
    c0, g0, H0, _ = O.accumulate(rec_out[40:], st[40:], 1.0, np.zeros(6))
    c1, g1, H1, _ = O.accumulate(rec_out, st, 1.0, np.zeros(6))
    assert np.allclose(g0, g1, rtol=0, atol=1e-9) and np.allclose(H0, H1, rtol=0, atol=1e-9)
    assert abs((c1 - c0) - 40 * 0.5 / 3.0) < 1e-9  # each saturated block costs rho = a^2/3
    pose, w, summ, costs = O.lm_solve(rec, st, 5.0, np.eye(4), two_d=True)
    assert w[2] == 0 and w[3] == 0 and w[4] == 0  # Z, rX, rY held constant


def test_covariance_is_the_inverse_information(O):
    rec, st, T = make_plane_problem()
    cov, err = O.covariance(rec, st, 5.0, T)
    c, g, H, _ = O.accumulate(rec, st, 5.0, np.array([0.3, -0.2, 0.1, 0.01, -0.02, 0.03]))
    assert np.allclose(cov @ H, np.eye(6), atol=1e-6)
    assert err[0] > 0 and err[1] > 0


# ---------------------------------------------------------------- extractor
def test_extractor_invariants(O, L):
    pts, _ = L.synth_frame(16, 1000, 0)
    ex = O.Extractor()
    counts = ex.compute(pts)
    lab = [ex.debug(4 + k).astype(bool) for k in range(3)]
    val = [ex.debug(7 + k).astype(bool) for k in range(3)]
    assert counts.tolist() == [int(l.sum()) for l in lab]
    for k in range(3):
        assert np.all(val[k][lab[k]])  # labelled points get their validity bit back (SSKE.cxx:584)
    ring = pts["laser_id"]
    for r in np.unique(ring):
        sel = np.flatnonzero(ring == r)
        pl = np.flatnonzero(lab[1][sel])
        assert np.all(np.diff(pl) > 4)  # plane NMS window +-4
        bl = np.flatnonzero(lab[2][sel])
        assert np.all(bl % 3 == 0)
        assert not lab[0][sel][:4].any() and not lab[0][sel][-4:].any()  # first/last NeighborWidth points are invalid
    # keypoint clouds are ring-major, index ascending
    for k in range(3):
        kp = ex.keypoints(k)
        assert np.all(np.diff(kp["laser_id"].astype(int)) >= 0)
    assert 0.003 < ex.azimuthal_resolution < 0.004  # 0.2 deg


def test_extractor_edge_cases(O, L):
    pts, _ = L.synth_frame(8, 1000, 0)
    ex = O.Extractor()
    ex.azimuthal_resolution = 0.0157
    few = pts[pts["laser_id"] == 0][:8]  # a ring with fewer than 2W+1 points: fully invalid
    assert ex.compute(few).tolist() == [0, 0, 0] and ex.debug(7).sum() == 0
    only7 = pts[pts["laser_id"] == 7]  # rings 0..6 empty
    c = ex.compute(only7)
    assert ex.nb_rings() == 8 and c[2] > 0
    dup = np.repeat(pts[pts["laser_id"] == 3], 2)  # dual returns hitting the same point: zero-length segments
    c = ex.compute(dup)
    assert np.isfinite(ex.debug(0)).all()
    one = pts[:1]
    assert ex.compute(one).tolist() == [0, 0, 0]


# ---------------------------------------------------------------- pipeline
def test_oracle_recovers_the_synthetic_motion(O, L):
    s = O.Slam(EgoMotion=3)
    prev = None
    steps = []
    for f in range(8):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
        T = s.world_transform()
        if prev is not None and f >= 4:
            steps.append(pose_diff(prev, T)[0])
        prev = T
    # 5 m/s at 10 Hz: every frame moves 0.5 m (the first frames carry the un-undistorted first sweep: transient)
    assert np.all(np.abs(np.array(steps) - 0.5) < 0.06), steps
    st = s.stats()
    assert st[12] > 1000 and st[13] >= 6  # matched keypoints, keyframes


def test_frame_checks(O, L):
    s = O.Slam(EgoMotion=3)
    pts, stamp = L.synth_frame(8, 1000, 0)
    s.add_frame(pts, 0, 0)  # stamp 0 equals the post-reset "previous" stamp: dropped (Slam.cxx:727-731)
    assert s.stats()[0] == 0
    s.add_frame(pts, stamp, 0)
    T0 = s.world_transform()
    s.add_frame(pts, stamp, 1)  # same stamp again: ignored
    assert np.array_equal(T0, s.world_transform())
    s.add_frame(pts[:0], stamp + 100000, 2)  # empty frame: ignored
    assert np.array_equal(T0, s.world_transform())


def test_lcp_estimator_properties(O, L):
    """Confidence::LCPEstimator (ConfidenceEstimators.cxx:27-65): 1 for a cloud lying on its map, ~0 far away,
    the best map wins, -1 when there is nothing to estimate."""
    pts, _ = L.synth_frame(8, 1000, 0)
    cloud = pts[:3000]
    far = cloud.copy()
    far["z"] += 500.0
    leaves = (0.3, 0.6, 0.3)
    assert O.lcp(cloud, 0.5, [cloud, None, None], leaves) == 1.0
    assert O.lcp(cloud, 0.5, [far, None, None], leaves) < 1e-6
    assert O.lcp(cloud, 0.5, [far, cloud, None], leaves) == 1.0  # best probability over the maps
    shifted = cloud.copy()
    shifted["z"] += 0.1  # one sigma of the 0.3 m leaf: exp(-0.5) at most, less where another point is nearer
    v = O.lcp(shifted, 1.0, [cloud, None, None], leaves)
    assert np.exp(-0.5) - 1e-6 <= v < 1.0
    assert O.lcp(cloud, 0.5, [None, None, None], leaves) == -1.0
    assert O.lcp(cloud[:1], 0.5, [cloud, None, None], leaves) == -1.0  # int(1 * 0.5) == 0 sampled points


def test_velodyne_conversion_properties(O, L):
    """VelodyneToLidarNode::Callback + SpinningFrameAdvancementEstimator: fields carried over, ring mapping, and
    a time built from the azimuth that grows monotonically inside every ring over about one revolution."""
    vel = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad", "<f4"), ("intensity", "<f4"), ("ring", "<u2"), ("pad2", "<u2"),
                    ("time", "<f4"), ("pad3", "<f4")])
    layout = (32, 0, 4, 8, 16, 20, 24)
    pts, _ = L.synth_frame(8, 1000, 1)
    rec = np.zeros(pts.size, vel)
    for f in ("x", "y", "z", "intensity"):
        rec[f] = pts[f]
    rec["ring"] = pts["laser_id"]
    rec["time"] = pts["time"].astype(np.float32)
    out, valid = O.velodyne_to_lidar(rec, layout, None, 2)
    assert valid and np.array_equal(out["x"], pts["x"]) and np.array_equal(out["laser_id"], pts["laser_id"])
    assert np.array_equal(out["time"], rec["time"].astype(np.float64)) and (out["device_id"] == 2).all() and (out["w"] == 1).all()
    mapping = np.arange(8, dtype=np.uint16)[::-1].copy()
    out2, _ = O.velodyne_to_lidar(rec, layout, mapping, 0)
    assert np.array_equal(out2["laser_id"], mapping[pts["laser_id"]])
    rec["time"] = 0
    for first, lo, hi in ((True, 0.0, 0.1), (False, -0.1, 0.0)):
        out3, valid = O.velodyne_to_lidar(rec, layout, None, 0, 600.0, first)
        assert not valid
        assert out3["time"][0] == lo and out3["time"].min() >= lo - 1e-12 and out3["time"].max() <= hi + 0.01
        for r in range(8):
            t = out3["time"][out3["laser_id"] == r]
            assert (np.diff(t) >= 0).all()  # the estimator's whole point: no wrap inside a ring


def test_oracle_pose_log_motion_limits_and_latency_compensation(O, L):
    """Slam.cxx:555-605, 1225-1264, 1391-1484 restated: log lengths for the three LoggingTimeout regimes, the motion
    limits around the synthetic sensor's 5 m/s, and the constant-velocity extrapolation by the latency."""
    runs = {}
    for timeout in (0.0, 0.35, -1.0):
        s = O.Slam(EgoMotion=3, LoggingTimeout=timeout, TimeWindowDuration=0.25, VelocityLimitLinear=4.0 if timeout < 0 else 6.0, VelocityLimitAngular=1e3)
        comply = []
        for f in range(8):
            pts, stamp = L.synth_frame(8, 1000, f)
            s.add_frame(pts, stamp, f)
            comply.append(s.debug_information()["Confidence: comply motion limits"])
        runs[timeout] = (s, comply)
    poses0, times0, cov0 = runs[0.0][0].trajectory()
    assert poses0.shape[0] == 2 and np.all(cov0 == 0)  # logging off: two poses for the extrapolation, no covariances
    poses1, times1, cov1 = runs[0.35][0].trajectory()
    assert poses1.shape[0] == 4 and np.allclose(times1[-1] - times1[0], 0.3) and np.any(cov1[-1] != 0)
    poses2, times2, _ = runs[-1.0][0].trajectory()
    assert poses2.shape[0] == 8 and np.array_equal(poses2[-2:], poses0)
    assert runs[0.0][1][2:] == [1.0] * 6      # 5 m/s under a 6 m/s limit
    assert runs[-1.0][1][2:] == [0.0] * 6     # ... and over a 4 m/s limit
    s = runs[-1.0][0]
    assert np.allclose(s.latency_compensated_world_transform(), poses2[-1], atol=1e-14, rtol=0)  # latency 0 (through a quaternion)
    s.set_param("Latency", 0.05)
    ahead = s.latency_compensated_world_transform()
    v = (poses2[-1][:3, 3] - poses2[-2][:3, 3]) / (times2[-1] - times2[-2])
    assert np.allclose(ahead[:3, 3], poses2[-1][:3, 3] + 0.05 * v, atol=1e-12)
    s.set_param("Latency", 1.0)  # more than MaxExtrapolationRatio x the frame period: no extrapolation
    assert np.array_equal(s.latency_compensated_world_transform(), poses2[-1])


def test_oracle_two_lidar_devices_merge_into_one_frame(O, L):
    """Slam::AddFrames with one frame per device (Slam.cxx:753-801, 1512-1578): the keypoints of the two devices are
    merged in frame order in BASE coordinates with times relative to the first stamp, the pose follows the synthetic
    motion as with the undivided scan, and the registered frame holds every input point."""
    s2, s1 = O.Slam(EgoMotion=3), O.Slam(EgoMotion=3)
    for f in range(6):
        frames, stamps, offset = two_device_rig(L, f)
        if f == 0:
            s2.set_base_to_lidar_offset(offset, device_id=1)
        s2.add_frames(frames, stamps, f)
        pts, stamp = L.synth_frame(8, 1000, f)
        s1.add_frame(pts, stamp, f)
        dt, dr = pose_diff(s2.world_transform(), s1.world_transform())
        assert dt < 0.05 and dr < 0.01, (f, dt, dr)  # same scene, rings split between two extractors
        kp = s2.keypoints(L.PLANE, 2)
        n0 = int((kp["device_id"] == 0).sum())
        assert 0 < n0 < kp.size and np.all(kp["device_id"][:n0] == 0) and np.all(kp["device_id"][n0:] == 1)
        assert kp["time"].min() >= -0.1001 and kp["time"].max() <= 1e-9
        # in BASE the second device's keypoints lie in the same street canyon as the first one's
        assert abs(np.median(kp["y"][n0:]) - np.median(kp["y"][:n0])) < 3.0
        reg = s2.registered_frame()
        assert reg.size == frames[0].size + frames[1].size
    # a device without extractor while another device has one: its frame is ignored (Slam.cxx:774-779)
    s3 = O.Slam(EgoMotion=3)
    s3.set_extractor_param(2, "NeighborWidth", 4)
    frames, stamps, offset = two_device_rig(L, 0)
    s3.add_frames(frames, stamps, 0)
    assert np.all(s3.keypoints(L.PLANE, 2)["device_id"] == 0)
    assert s3.registered_frame().size == frames[0].size + frames[1].size


# ---------------------------------------------------------------- hand-derived cases for the restated Ceres pieces
def one_record(A=np.eye(3), P=(0, 0, 0), X=(0, 0, 0), weight=1.0):
    rec = np.zeros((1, 16))
    rec[0, :9], rec[0, 9:12], rec[0, 12:15], rec[0, 15] = np.asarray(A, float).reshape(9), P, X, weight
    return rec, np.zeros(1, np.uint8)


def test_tukey_scaled_loss_by_hand(O):
    """ScaledLoss(TukeyLoss(a), w) as KeypointsMatcher.cxx:96-101 builds it for Ceres >= 2 -- rho(s) = a^2/3 (1 - (1 - s/a^2)^3)
    inside, a^2/3 outside, times w -- and what the corrector makes of it when rho'' <= 0: cost = rho / 2, g = rho' J^T r,
    H = rho' J^T J.  One residual block, A = I, X = 0, so r = t - P and J_t = I: numbers a pencil can follow."""
    a, w = 2.0, 0.75
    # (i) saturated: |r|^2 = 9 > a^2 = 4
    rec, st = one_record(P=(3, 0, 0), weight=w)
    c, g, H, nv = O.accumulate(rec, st, a, np.zeros(6))
    assert nv == 1 and c == 0.5 * w * a * a / 3.0 and not g.any() and not H.any()
    # (ii) inside, s = |r|^2 = 2 = a^2 / 2: rho = a^2/3 (1 - 1/8), rho' = (1 - 1/2)^2 = 1/4
    rec, st = one_record(P=(-np.sqrt(2.0), 0, 0), weight=w)
    c, g, H, nv = O.accumulate(rec, st, a, np.zeros(6))
    s = np.sqrt(2.0) ** 2
    rho, drho = a * a / 3.0 * (1 - (1 - s / (a * a)) ** 3), (1 - s / (a * a)) ** 2
    assert abs(c - 0.5 * w * rho) < 1e-15 and abs(g[0] - w * drho * np.sqrt(2.0)) < 1e-15 and not g[1:3].any()
    assert np.allclose(H[:3, :3], w * drho * np.eye(3), rtol=0, atol=1e-15)
    # (iii) on the boundary s = a^2 the two branches agree (rho = a^2/3, rho' = 0)
    rec, st = one_record(P=(a, 0, 0), weight=w)
    c, g, H, _ = O.accumulate(rec, st, a, np.zeros(6))
    assert abs(c - 0.5 * w * a * a / 3.0) < 1e-15 and np.abs(g).max() < 1e-15


def test_residual_jacobian_by_hand(O):
    """MahalanobisDistanceAffineIsometryResidual (CeresCostFunctions.h:105-152) with R = Rz(rz) Ry(ry) Rx(rx) (:67-79),
    parameters (x, y, z, rx, ry, rz): at rpy = 0 and X = (1, 0, 0), d(R X)/drx = 0, d/dry = (0, 0, -1), d/drz = (0, 1, 0).
    With A = I, P = X + (0, 0.1, 0), t = 0: r = (0, -0.1, 0).  Far below the saturation distance (a = 100: rho' = (1 - s / a^2)^2 = 1 to 1e-5)."""
    rec, st = one_record(P=(1, 0.1, 0), X=(1, 0, 0))
    c, g, H, _ = O.accumulate(rec, st, 100.0, np.zeros(6))
    J = np.array([[1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 1], [0, 0, 1, 0, -1, 0]], float)
    r = np.array([0, -0.1, 0])
    assert np.allclose(g, J.T @ r, rtol=0, atol=1e-5) and np.allclose(H, J.T @ J, rtol=0, atol=1e-5) and abs(c - 0.5 * 0.01) < 1e-6
    # a quarter turn about z: R X = (0, 1, 0); d/drz = (-1, 0, 0), d/dry = Rz (0, 0, -1) = (0, 0, -1), d/drx = 0 (X on the x axis)
    w6 = np.array([0, 0, 0, 0, 0, np.pi / 2])
    rec, st = one_record(P=(0, 1, 0.2), X=(1, 0, 0))
    c, g, H, _ = O.accumulate(rec, st, 100.0, w6)
    J = np.array([[1, 0, 0, 0, 0, -1], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, -1, 0]], float)
    r = np.array([0, 0, -0.2])
    assert np.allclose(g, J.T @ r, rtol=0, atol=1e-5) and np.allclose(H, J.T @ J, rtol=0, atol=1e-5)
    # a point-to-plane block: A = n n^T projects onto the normal, so only motion along n is seen
    n = np.array([0, 0, 1.0])
    rec, st = one_record(A=np.outer(n, n), P=(5, 5, 1), X=(0, 0, 0))
    c, g, H, _ = O.accumulate(rec, st, 100.0, np.zeros(6))
    assert abs(c - 0.5) < 1e-3 and np.allclose(g[:3], [0, 0, -1], atol=1e-3) and np.allclose(H[:3, :3], np.outer(n, n), atol=1e-3)


def test_lm_on_a_linear_least_squares_problem_by_hand(O):
    """Point-to-point blocks (A = I, X = 0) far below the saturation distance: cost = 1/2 sum |t - P_i|^2, minimum at the
    mean of the P_i, H = N I exactly, and the first trust-region step of Ceres' Levenberg-Marquardt (radius 1e4, Jacobi
    scaling, LocalOptimizer.cxx:93-96 leaves the defaults) is the Gauss-Newton step shortened by 1 / (1 + 1e-4 ...): the
    solver must arrive within a few steps, report them, and stop by a tolerance, not by the iteration cap."""
    rng = np.random.default_rng(7)
    P = rng.normal(size=(50, 3)) + [1.0, -2.0, 0.5]
    rec = np.zeros((50, 16))
    rec[:, [0, 4, 8]] = 1.0
    rec[:, 9:12] = P
    rec[:, 15] = 1.0
    st = np.zeros(50, np.uint8)
    c, g, H, _ = O.accumulate(rec, st, 1e4, np.zeros(6))
    assert np.allclose(H[:3, :3], 50 * np.eye(3), atol=1e-3) and np.allclose(g[:3], -P.sum(0), atol=1e-3) and not H[3:, 3:].any()
    pose, w, summ, costs = O.lm_solve(rec, st, 1e4, np.eye(4), max_iter=15, two_d=False)
    mean = P.mean(0)
    # H is diagonal here, so is the damped system: (H + diag(H) / radius) step = -g with radius = 1e4 gives the
    # Gauss-Newton step divided by (1 + 1e-4).  The second iteration's candidate changes the cost by less than
    # function_tolerance (1e-6) x cost: Ceres stops WITHOUT taking it.  So the answer is the mean short of 1e-4, exactly.
    assert np.abs(w[:3] - mean / (1 + 1e-4)).max() < 1e-7, (w, mean)
    assert summ[0] == 2 and summ[2] == 2  # one accepted step (+ iteration 0), two iterations
    assert abs(costs[1] - 0.5 * ((P - mean) ** 2).sum()) < 1e-4


def test_libm_instead_of_the_portable_trigonometry(O, L, golden, capsys):
    """Parity with the reference is unpinned at one more place than the missing fixtures: include/lsa_pmath.h is compiled
    into BOTH the oracle and the kernels, so the atan2 / cos / sin inside pcl::eigen33 can never disagree between the two
    while both may differ from glibc (the reference) in the last ulp.  This runs the oracle with glibc's functions in the
    eigen-solver and the slerp and counts what changes: low bits of scores, and DECISIONS (keypoint labels, validity,
    match status).  The counts are reported (DESIGN.md 4.1 holds them); decisions must be all but untouched."""
    frames = [golden[f"frame{f}"] for f in range(4)] + [L.synth_frame(16, 1000, f)[0] for f in range(3)]
    report = {"points": 0, "score_values_differing": 0, "label_or_validity_flips": 0, "keypoints": 0, "match_status_flips": 0, "matches": 0,
              "weight_values_differing": 0}
    results = {}
    for libm in (0, 1):
        O.set_libm_trig(libm)
        try:
            ex = O.Extractor()
            per_frame = []
            for pts in frames:
                ex.compute(pts)
                per_frame.append(([ex.debug(i).copy() for i in range(10)], [ex.keypoints(k).copy() for k in range(3)]))
            matches = []
            for a, b in ((0, 1), (4, 5), (5, 6)):
                T = np.eye(4)
                T[0, 3] = 0.45
                for k in range(3):
                    for mp in (L.MatchParams.ego_motion(saturation_distance=5.0), L.MatchParams.localization(saturation_distance=2.0)):
                        matches.append(O.match(per_frame[b][1][k], per_frame[a][1][k], k, mp, T)[:2])
            s = O.Slam(EgoMotion=3)
            for f in range(3):
                pts, stamp = L.synth_frame(16, 1000, f)
                s.add_frame(pts, stamp, f)
            results[libm] = (per_frame, matches, s.world_transform())
        finally:
            O.set_libm_trig(0)
    for (dbg0, kp0), (dbg1, kp1) in zip(results[0][0], results[1][0]):
        report["points"] += dbg0[0].size
        for i in range(4):
            report["score_values_differing"] += int((dbg0[i].view(np.uint32) != dbg1[i].view(np.uint32)).sum())
        for i in range(4, 10):
            report["label_or_validity_flips"] += int((dbg0[i] != dbg1[i]).sum())
        report["keypoints"] += sum(k.size for k in kp0)
    for (st0, w0), (st1, w1) in zip(results[0][1], results[1][1]):
        if st0.size == st1.size:
            report["matches"] += st0.size
            report["match_status_flips"] += int((st0 != st1).sum())
            report["weight_values_differing"] += int((w0.view(np.uint64) != w1.view(np.uint64)).sum())
    dp, da = pose_diff(results[0][2], results[1][2])
    report["pose_difference_after_3_frames"] = [dp, da]
    with capsys.disabled():
        print("\nlibm vs lsa_pmath in the oracle:", report)
    assert report["label_or_validity_flips"] <= 2 and report["match_status_flips"] <= 2
    assert dp < 1e-6 and da < 1e-6


def test_robosense_conversion_follows_the_driver_nodes_loop(O):
    """orc_robosense_to_lidar against the reference's loop written out in Python, rule by rule (wire_cases.robosense_node,
    ros_wrapping/lidar_conversions/src/RobosenseToLidarNode.cxx:78-121), byte for byte: NaN records skipped, a record equal to the last
    point KEPT skipped, laser_id = i / width through RS16's mapping when the cloud has 16 rows, time from i mod (size / rows)"""
    from wire_cases import robosense_node

    RS = np.dtype({"names": ["x", "y", "z", "intensity"], "formats": ["<f4"] * 4, "offsets": [0, 4, 8, 16], "itemsize": 32})
    rng = np.random.default_rng(0)
    for h, w, mapping in ((16, 50, None), (12, 40, None), (16, 30, list(range(15, -1, -1)))):
        rec = np.zeros(h * w, RS)
        for c in ("x", "y", "z", "intensity"):
            rec[c] = rng.normal(size=h * w).astype(np.float32)
        rec["x"][rng.random(h * w) < 0.1] = np.nan
        d = np.nonzero(rng.random(h * w) < 0.2)[0]
        d = d[d > 0]
        for c in "xyz":
            rec[c][d] = rec[c][d - 1]
        out = O.robosense_to_lidar(rec, w, h, (32, 0, 4, 8, 16), mapping, 2, 600.0)
        want = robosense_node(rec.view(np.uint8), w, h, (32, 0, 4, 8, 16), mapping, 2, 600.0)
        assert 0 < want.size < h * w and out.tobytes() == want.tobytes()


# ---------------------------------------------------------------- pose algebra between two ICP iterations
def test_the_products_pose_algebra_is_the_restatements_bit_for_bit(O, L):
    """What the product does between two ICP iterations -- on the host (lsa_posemath.h) and, from the same source, on the
    device behind a solve (lsa_icp_link) -- against the oracle's own restatement of Utils::XYZRPYtoIsometry /
    IsometryToXYZRPY (Utilities.cxx:33-77), Slam::InterpolateScanPose / RefineUndistortion (Slam.cxx:1271-1285, 1322-1352),
    LinearInterpolation (MotionModel.cxx:26-34) and LinearTransformInterpolator (MotionModel.h:36-136): two independent
    write-ups of the same arithmetic must give the same bits.  (tests/test_gpu_match.py holds the device's block against
    the host's.)  No GPU needed: lsa_icp_link_expected is host code."""
    rng = np.random.default_rng(17)

    def se3(w):
        cx, cy, cz = np.cos(w[3:]); sx, sy, sz = np.sin(w[3:])
        T = np.eye(4)
        T[:3, :3] = np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz], [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz], [-sy, sx * cy, cx * cy]])
        T[:3, 3] = w[:3]
        return T

    def unit(q):
        return q / np.linalg.norm(q)

    cases = 0
    for trial in range(400):
        big = trial % 5 == 4  # every fifth case: rotations of any size (the quaternion conversion's trace <= 0 branches, yaw near pi)
        x = np.concatenate([rng.normal(0, 30, 3), rng.uniform(-np.pi, np.pi, 3) if big else rng.normal(0, 0.05, 3)])
        if big:
            x[4] = rng.uniform(-1.5, 1.5)  # pitch inside (-pi / 2, pi / 2), as the reference's conversion assumes
        prev = se3(np.concatenate([x[:3] + rng.normal(0, 0.5, 3), x[3:] + rng.normal(0, 0.02 if not big else 1.0, 3)]))
        have_log = trial % 7 != 0
        ratio = 0.5 if trial % 11 == 0 else 3.0
        t0, t1 = (0.0, 0.0) if trial % 13 == 0 else (-0.1, -1e-4 * (trial % 3))
        if trial % 17 == 0:
            q0 = q1 = np.array([1.0, 0.0, 0.0, 0.0])  # the motion as InitUndistortion leaves it
            tr0 = tr1 = np.zeros(3)
        else:
            q0, q1 = unit(rng.normal(0, 1e-2 if not big else 1.0, 4) + [1, 0, 0, 0]), unit(rng.normal(0, 1e-2 if not big else 1.0, 4) + [1, 0, 0, 0])
            tr0, tr1 = rng.normal(0, 0.05, 3), rng.normal(0, 0.05, 3)
        motion = np.concatenate([[t0, t1], q0, q1, tr0, tr1])
        for refine in (0, 1):
            ln = L.IcpLink()
            ln.refine_undistortion, ln.first, ln.have_log = refine, 1, int(have_log)
            ln.prev_time, ln.cur_time, ln.max_extrapolation_ratio = 10.0, 10.1, ratio
            ln.previous_world[:] = list(prev.reshape(-1))
            ln.motion[:] = list(motion)
            got, got_motion = L.icp_link_expected(x, 0, 2, ln)
            want, want_motion = O.icp_link(x, refine, have_log, 10.0, 10.1, ratio, prev, motion)
            n = 19 if not refine else 51
            assert np.array_equal(got[:n], want[:n]), (trial, refine, np.nonzero(got[:n] != want[:n])[0])
            assert np.array_equal(got_motion.view(np.uint64), want_motion.view(np.uint64)), (trial, refine)
            cases += 1
    assert cases == 800
    # a solve that was skipped, or made no step, leaves "do not run"
    assert L.icp_link_expected(x, 1, 3, ln)[0][0] == 0 and L.icp_link_expected(x, 0, 1, ln)[0][0] == 0
