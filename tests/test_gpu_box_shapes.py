"""The keypoint boxes and time ranges of lsa_transform.hip (k_bbox3, k_time_range3, k_loc_start) at the sizes where a
wavefront or a workgroup ends: the pipeline only ever feeds them whole frames.

One keypoint type gets n points, one none, one n + 64; the extreme coordinates and times sit at index 0 and at the last
index of a type -- the first lane of its first wavefront and the last live lane of its last.  The reference is numpy: min / max
per coordinate in float32 over the points that take part, min / max of the times in float64.  Under the identity a point moves
onto itself exactly (1 * x + 0 * y + 0 * z + 0 in double); under the fixed pose the reference is the min / max of
transformed_keypoints, the device's own arithmetic, which test_gpu_pipeline.py holds bit for bit to the oracle.  A pose mixes
the coordinates (0 * NaN = NaN), so a point with one NaN coordinate takes no part in any coordinate of the box.  Equality by
value, no tolerance; a type without points reports FLT_MAX / -FLT_MAX."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 1025]
BIG = np.finfo(np.float32).max


def fixed_pose():
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(0.7) * K + (1 - np.cos(0.7)) * (K @ K)
    T[:3, 3] = [12.5, -3.25, 0.75]
    return T


@pytest.fixture(scope="module")
def ctx(L):
    c = L.Context(0)  # its own: lsa_localization_begin leaves state behind
    yield c
    c.close()


def cloud(L, rng, n, reach, t_lo, t_hi):
    """n random points; index 0 holds the smallest x, y, z and time, index n - 1 the largest"""
    p = np.zeros(n, L.POINT_DTYPE)
    for c in "xyz":
        p[c] = rng.uniform(-50, 50, n).astype(np.float32)
    p["w"] = 1.0
    p["time"] = rng.uniform(-0.1, 0.0, n)
    p["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
    p["laser_id"] = rng.integers(0, 16, n)
    if n:
        for c in "xyz":
            p[c][n - 1] = reach
        p["time"][n - 1] = t_hi
        for c in "xyz":  # (n = 1: the one point is the smallest and the largest)
            p[c][0] = -reach if n > 1 else reach
        p["time"][0] = t_lo if n > 1 else t_hi
    return p


def box_of(pts):
    """min / max per coordinate over the points without a NaN coordinate, in float32"""
    lo, hi = np.full(3, BIG, np.float32), np.full(3, -BIG, np.float32)
    ok = ~(np.isnan(pts["x"]) | np.isnan(pts["y"]) | np.isnan(pts["z"]))
    if ok.any():
        for d, c in enumerate("xyz"):
            lo[d], hi[d] = np.nanmin(pts[c][ok]), np.nanmax(pts[c][ok])
    return lo, hi


@pytest.mark.parametrize("with_nan", [False, True], ids=["clean", "nan"])
@pytest.mark.parametrize("n", SIZES)
def test_boxes_and_time_range_where_wavefronts_and_workgroups_end(L, ctx, n, with_nan):
    idx = SIZES.index(n)
    rng = np.random.default_rng(20261019 + 2 * idx + int(with_nan))
    small, empty, large = idx % 3, (idx + 1) % 3, (idx + 2) % 3  # which type has n points, none, n + 64
    sets = [None] * 3
    # the set's extreme times: in the n-point type at every other size, in the other one otherwise
    far = idx % 2 == 0
    sets[small] = cloud(L, rng, n, 60.0, -0.2 if far else -0.15, 0.05 if far else 0.04)
    sets[empty] = np.zeros(0, L.POINT_DTYPE)
    sets[large] = cloud(L, rng, n + 64, 70.0, -0.15 if far else -0.2, 0.04 if far else 0.05)
    if with_nan:
        # the point that holds the minima drops out; (n = 1: in the other type, a type of NaN points only has no box to state)
        victim = small if n > 1 else large
        sets[victim]["xyz"[idx % 3]][0] = np.nan
    for k in range(3):
        ctx.set_keypoints(L.SET_RAW_CURRENT, k, sets[k])

    def check(mn, mx, want):
        for k in range(3):
            lo, hi = want[k]
            print(n, with_nan, k, mn[k], lo, mx[k], hi)
            assert np.array_equal(mn[k], lo) and np.array_equal(mx[k], hi)

    # 1. the boxes under the identity: the points themselves
    mn, mx = ctx.keypoint_bboxes(L.SET_RAW_CURRENT, np.eye(4))
    check(mn, mx, [box_of(sets[k]) for k in range(3)])

    # 2. under a pose: the device's own moved points
    T = fixed_pose()
    moved = [box_of(ctx.transformed_keypoints(L.SET_RAW_CURRENT, k, T)) for k in range(3)]
    assert np.all(moved[empty][0] == BIG) and np.all(moved[empty][1] == -BIG)
    mn, mx = ctx.keypoint_bboxes(L.SET_RAW_CURRENT, T)
    check(mn, mx, moved)

    # 3. the time range of the set
    times = np.concatenate([s["time"] for s in sets])
    assert times.dtype == np.float64
    t0, t1 = ctx.keypoint_time_range(L.SET_RAW_CURRENT)
    print(n, with_nan, t0, times.min(), t1, times.max())
    assert t0 == times.min() and t1 == times.max()

    # 4. the localization's start: working = raw (no undistortion), the boxes under the pose in the same launch
    ctx.reset_working_keypoints()
    ctx.localization_begin(box_pose=T, arm=True)
    mn, mx = ctx.keypoint_bboxes_end()
    check(mn, mx, moved)
    for k in range(3):
        assert ctx.keypoints(L.SET_WORKING, k).tobytes() == sets[k].tobytes()
