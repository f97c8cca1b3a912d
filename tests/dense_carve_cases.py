"""Cases for the dense map's free-space carving (lidarslam_amd/_dense_map.py: DenseMapHost.carve, dense_ray_steps;
lidarslam_amd/csrc/lsa_dense_carve.hip: k_dense_carve).  Needs neither a GPU nor the native library.

As in tests/dense_map_cases.py the leaf is 0.5 and most coordinates are multiples of 0.125, so that rays start and end on voxel
corners, edges and faces on purpose.  A ray case is (origin, point, keyword arguments of carve); `walk` is the list of voxels
DenseMapHost's walk visits for it, or None when the definition casts no ray."""
import numpy as np

from dense_map_cases import LEAF, cloud
from lidarslam_amd._dense_map import DENSE_INDEX_RANGE, DenseMapHost, dense_ray_steps

F32 = np.float32
ONE_DOWN, ONE_UP = float(np.nextafter(F32(1), F32(0))), float(np.nextafter(F32(1), F32(2)))
EDGE = DENSE_INDEX_RANGE * LEAF  # the first coordinate past the index range

# name -> (origin, point, carve keywords).  margin_leaves = 0 makes the ray end in the point itself.
RAY_CASES = {
    # the six axis directions: two components exactly 0
    "axis+x": ((0.125, 0.125, 0.125), (3.125, 0.125, 0.125), {}),
    "axis-x": ((0.125, 0.125, 0.125), (-2.875, 0.125, 0.125), {}),
    "axis+y": ((0.125, 0.125, 0.125), (0.125, 3.125, 0.125), {}),
    "axis-y": ((0.125, 0.125, 0.125), (0.125, -2.875, 0.125), {}),
    "axis+z": ((0.125, 0.125, 0.125), (0.125, 0.125, 3.125), {}),
    "axis-z": ((0.125, 0.125, 0.125), (0.125, 0.125, -2.875), {}),
    # origin and end on voxel corners and edges: every tmax ties (TIES holds the visits written out by hand)
    "corner+": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), {"margin_leaves": 0.0}),
    "corner-": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), {"margin_leaves": 0.0}),
    "edge": ((0.5, 0.5, 0.125), (1.5, 1.5, 0.125), {"margin_leaves": 0.0}),
    "edge_yz": ((0.125, 1.0, -0.5), (0.125, 0.0, 0.5), {"margin_leaves": 0.0}),
    # crossing 0 on every axis
    "through_zero": ((-1.3, -0.7, -0.4), (2.1, 1.9, 0.8), {}),
    "through_zero_back": ((1.3, 0.7, 0.4), (-2.1, -1.9, -0.8), {"margin_leaves": 0.5}),
    # start and end in one voxel
    "one_voxel": ((0.1, 0.1, 0.1), (0.3, 0.2, 0.15), {"margin_leaves": 0.0}),
    # len just under, at and just over the margin (2 leaves = 1.0)
    "under_margin": ((0.0, 0.0, 0.0), (ONE_DOWN, 0.0, 0.0), {}),
    "at_margin": ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), {}),
    "over_margin": ((0.0, 0.0, 0.0), (ONE_UP, 0.0, 0.0), {}),
    # longer than the range
    "long": ((0.1, 0.2, 0.3), (40.0, 5.0, -3.0), {}),
    "short_range": ((0.1, 0.2, 0.3), (4.0, 5.0, -3.0), {"max_range": 2.0}),
    # non-finite
    "nan_origin": ((np.nan, 0.0, 0.0), (3.0, 0.0, 0.0), {}),
    "inf_point": ((0.0, 0.0, 0.0), (3.0, np.inf, 0.0), {}),
    # indices out of range: the start, the end, and a ray that just stays inside
    "start_outside": ((EDGE, 0.0, 0.0), (EDGE - 8.0, 0.0, 0.0), {}),
    "end_outside": ((EDGE - 1.0, 0.0, 0.0), (EDGE + 12.0, 0.0, 0.0), {"margin_leaves": 0.0}),
    "stays_inside": ((EDGE - 8.0, 0.25, 0.25), (EDGE - 0.125, 0.25, 0.25), {"margin_leaves": 0.0}),
    "low_edge": ((-EDGE + 4.0, 0.25, 0.25), (-EDGE, 0.25, 0.25), {"margin_leaves": 0.0}),
}
NO_RAY = {"under_margin", "at_margin", "nan_origin", "inf_point", "start_outside", "end_outside"}

# written out by hand from the definition: the axis of smallest tmax, ties to x before y before z
TIES = {
    "corner+": [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2)],
    "corner-": [(2, 2, 2), (1, 2, 2), (1, 1, 2), (1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0)],
    "edge": [(1, 1, 0), (2, 1, 0), (2, 2, 0), (3, 2, 0), (3, 3, 0)],
    "edge_yz": [(0, 2, -1), (0, 1, -1), (0, 0, -1), (0, 0, 0), (0, 0, 1)],  # y and z tie at 0.5: y first
}


def ray(name):
    """(one LidarPoint, origin (1, 3) float32, keywords)"""
    o, p, kw = RAY_CASES[name]
    return cloud([p]), np.array([o], F32), kw


def walks(points, origins, leaf=LEAF, **kw):
    """per point of `points` the list of voxels its ray visits, None for a point that casts none"""
    out = [None] * len(points)
    for rays, index in dense_ray_steps(points, origins, leaf, **kw):
        for r, i in zip(rays.tolist(), index.tolist()):
            if out[r] is None:
                out[r] = []
            out[r].append(tuple(i))
    return out


def walk(name):
    pts, org, kw = ray(name)
    return walks(pts, org, **kw)[0]


def voxel_points(indices, first_index=0, leaf=LEAF):
    """one LidarPoint at the centre of every voxel index (n, 3)"""
    idx = np.asarray(indices, np.float64).reshape(-1, 3)
    return cloud((idx + 0.5) * leaf, first_index=first_index)


def around(indices, reach=1):
    """the voxel indices within `reach` (Chebyshev) of any of `indices`, inside the index range, sorted"""
    idx = np.asarray(indices, np.int64).reshape(-1, 3)
    g = np.arange(-reach, reach + 1)
    offsets = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    every = np.unique((idx[:, None, :] + offsets[None, :, :]).reshape(-1, 3), axis=0)
    return every[((every >= -DENSE_INDEX_RANGE) & (every < DENSE_INDEX_RANGE)).all(axis=1)]


def ray_scene(name):
    """voxels for a map the ray of case `name` is carved through: what the walk visits and everything next to it (a wrong
    path shows as a miss beside the right one); for a case without a ray, the surroundings of its finite end points"""
    o, p, _ = RAY_CASES[name]
    visited = walk(name)
    if visited is None:
        ends = [np.floor(np.asarray(v, np.float64) / LEAF) for v in (o, p) if np.isfinite(v).all()]
        visited = [np.clip(e, -DENSE_INDEX_RANGE, DENSE_INDEX_RANGE - 1) for e in ends]
    return voxel_points(around(visited))


# ---- the scene: a wall, and an object in front of it that goes away --------------------------------------------------------
SENSOR = np.array([[0.25, 0.25, 0.25]], F32)
SCENE_FRAMES = 8


def scene():
    """-> (calls [(points, frame)], wall voxel indices, object voxel indices).  The wall, 13 x 13 voxels at x index 12, is seen
    in all 8 frames.  The object, 2 x 2 x 2 voxels at x index 5 and 6, is there in frames 0 to 3 and moves one voxel in y a
    frame (a pedestrian): each of its voxels is hit in one or two frames and seen through by the wall's rays in the others.
    (One standing still for 4 frames and seen through in the other 4 has misses == frames and stays at ratio 1.)  At the
    object the wall's rays are 0.25 apart, half a voxel, so every object voxel is crossed."""
    g = np.arange(-6, 7)
    wall = np.stack(np.meshgrid([12], g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    calls, objects = [], []
    for f in range(SCENE_FRAMES):
        pts = voxel_points(wall, first_index=1000 * f)
        if f < 4:
            b = np.arange(2)
            block = np.stack(np.meshgrid(5 + b, f - 2 + b, -1 + b, indexing="ij"), axis=-1).reshape(-1, 3)
            objects.append(block)
            pts = np.concatenate([pts, voxel_points(block, first_index=1000 * f + 500)])
        calls.append((pts, f))
    return calls, wall, np.unique(np.concatenate(objects), axis=0)


def carved_scene(make, carve_kw=None):
    """the scene inserted and carved frame by frame into make(): insert, then carve, per ordinal"""
    calls, wall, obj = scene()
    m = make()
    for pts, f in calls:
        m.insert(pts, f) if hasattr(m, "insert") else m.insert_points(pts, f)
        if hasattr(m, "carve"):
            m.carve(pts, SENSOR, f, **(carve_kw or {}))
        else:
            m.carve_points(pts, SENSOR, f)
    return m, wall, obj


def host_scene():
    return carved_scene(lambda: DenseMapHost(LEAF))


RATIOS = (0.0, 0.5, 1.0, -1.0)


# ---- clouds of rays ----------------------------------------------------------------------------------------------------------
def ray_cloud(n, seed=0, reach=6.0):
    """n points around the origin, off the lattice, for rays from one origin; and a map's worth of voxels under them"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-reach, reach, size=(n, 3))
    return cloud(xyz.astype(F32), intensity=rng.integers(0, 200, n))


def mixed_wavefront():
    """64 rays: every other one stays in its voxel (0 steps), the others are as long as range / leaf allows, 4096 leaves.
    -> (points, origins (64, 3), leaf, range)"""
    leaf, max_range = 0.125, 0.125 * 4096
    rng = np.random.default_rng(5)
    o = np.zeros((64, 3), F32) + F32(0.03125)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = o + np.where(np.arange(64)[:, None] % 2 == 0, d * 0.02, d * (max_range + 5.0))
    return cloud(p.astype(F32)), o, leaf, max_range


def same_state(device, host, min_frames=1, max_miss_ratio=-1.0):
    """same() of tests/test_gpu_dense_map.py, extended by sources and misses; returns the number of voxels"""
    dp, dv = device.get(min_frames, max_miss_ratio)
    hp, hv = host.get(min_frames, max_miss_ratio)
    assert dv.tobytes() == hv.tobytes(), (len(dv), len(hv))
    assert dp.tobytes() == hp.tobytes()
    assert device.sources(min_frames, max_miss_ratio).tobytes() == host.sources(min_frames, max_miss_ratio).tobytes()
    dm, hm = device.misses(min_frames, max_miss_ratio), host.misses(min_frames, max_miss_ratio)
    assert dm.dtype == hm.dtype == np.uint32 and dm.tobytes() == hm.tobytes(), (int(dm.sum()), int(hm.sum()))
    return len(hv)
