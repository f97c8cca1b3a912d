"""Cases for the dense map's normals (lidarslam_amd/_dense_map.py: DenseMapHost.normals, dense_normals;
lidarslam_amd/csrc/lsa_dense_normals.hip: k_dense_normals).  Needs neither a GPU nor the native library.

A case is (leaf, steps, queries, device parameters): `steps` build the map -- ("insert", points, frame) and ("carve", points,
origins, frame), every carve with margin 0 --, and every query is a dict of keyword arguments of normals().  The host tests
(tests/test_dense_normals_host.py) assert what the definition must give; the GPU tests (tests/test_gpu_dense_normals.py) hold
the device to the host statement on every case and query, byte for byte.

As in tests/dense_map_cases.py the leaf is 0.5; the exact scenes have their points at voxel centres, multiples of 0.25, so
that every d, product and sum of the definition is exact."""
import numpy as np

from dense_carve_cases import SENSOR, voxel_points
from dense_map_cases import LEAF, cloud, distinct_voxels
from lidarslam_amd._dense_map import DENSE_INDEX_RANGE, DENSE_NO_NORMAL, DenseMapHost, dense_normal_dtype

LO, HI = -DENSE_INDEX_RANGE, DENSE_INDEX_RANGE - 1
FLOATS = ("normal_x", "normal_y", "normal_z", "curvature")
CARVE_KW = dict(margin_leaves=0.0, max_range=30.0, stride=1)
CARVE_PARAMS = dict(CarveMarginLeaves=0.0, CarveRange=30.0, CarveStride=1)


def grid(xs, ys, zs):
    return np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3)


def both_radii(**kw):
    return [dict(radius_leaves=r, **kw) for r in (1, 2)]


# ---- 1. exact scenes --------------------------------------------------------------------------------------------------------
PLANE = np.arange(-4, 5)  # 9 x 9 voxels across the -1 / 0 index boundary, at z index 3


def plane():
    return LEAF, [("insert", voxel_points(grid(PLANE, PLANE, [3])), 0)], both_radii(), {}


def row():
    """9 voxels in a row along x: exactly collinear, two eigenvalues are exactly 0 (the double-root branch)"""
    return LEAF, [("insert", voxel_points(grid(PLANE, [0], [0])), 0)], both_radii(min_neighbors=3), {}


def lone():
    return LEAF, [("insert", voxel_points([[7, -2, 1]]), 0)], both_radii(min_neighbors=3), {}


def plus():
    """a centre and its four face neighbours in the xy plane: the centre has k = 5, an arm k = 4 (r = 1)"""
    idx = [[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]]
    return LEAF, [("insert", voxel_points(idx), 0)], [dict(radius_leaves=1, min_neighbors=m) for m in (4, 5, 6)] + both_radii(), {}


def blocks():
    """a 7^3 block of voxels, the points off the centres: in its middle every cell of 3^3 and of 5^3 is found"""
    idx = grid(np.arange(-3, 4), np.arange(-3, 4), np.arange(-3, 4))
    rng = np.random.default_rng(2)
    xyz = (idx + rng.uniform(0.05, 0.95, idx.shape)) * LEAF
    return LEAF, [("insert", cloud(xyz.astype(np.float32)), 0)], both_radii() + [dict(radius_leaves=1, min_neighbors=27), dict(radius_leaves=2, min_neighbors=125)], {}


# ---- 2. orientation ---------------------------------------------------------------------------------------------------------
ABOVE, BELOW, LEVEL = [0.0, 0.0, 9.0], [0.0, 0.0, -9.0], [20.0, 20.0, 1.75]  # (1.75: the z of the plane's points, dot == 0)


def oriented():
    """the plane, a quarter of it measured by each of the ordinals 0..3"""
    idx = grid(PLANE, PLANE, [3])
    steps = [("insert", voxel_points(idx[f::4], first_index=100 * f), f) for f in range(4)]
    queries = []
    for r in (1, 2):
        queries += [
            dict(radius_leaves=r, viewpoints=[ABOVE]), dict(radius_leaves=r, viewpoints=[BELOW]), dict(radius_leaves=r, viewpoints=[LEVEL]),
            # sources 0..3 against entries for the ordinals 1 and 2: 0 is clamped up, 3 down
            dict(radius_leaves=r, viewpoints=[ABOVE, BELOW], first_frame=1), dict(radius_leaves=r, viewpoints=[BELOW, ABOVE], first_frame=1),
            dict(radius_leaves=r, viewpoints=np.zeros((0, 3), np.float32)), dict(radius_leaves=r),
        ]
    return LEAF, steps, queries, {}


# ---- 4. the predicate ---------------------------------------------------------------------------------------------------------
WALL = grid([12], np.arange(-4, 5), np.arange(-4, 5))
CLUSTER = grid([11], [0, 1], [0, 1])  # right in front of the wall


def low_frames(with_cluster=True):
    """a wall seen in four frames, and a cluster in front of it seen in the first alone: min_frames = 2 leaves it out"""
    steps = []
    for f in range(4):
        pts = voxel_points(WALL, first_index=1000 * f)
        if f == 0 and with_cluster:
            pts = np.concatenate([pts, voxel_points(CLUSTER, first_index=500)])
        steps.append(("insert", pts, f))
    return LEAF, steps, both_radii(min_frames=2, min_neighbors=4) + both_radii(min_neighbors=4), {}


def seen_through(with_cluster=True):
    """the cluster is hit in frames 0 and 1 and seen through by the wall's rays in frames 2..7: misses 6 > frames 2"""
    steps = []
    for f in range(8):
        pts = voxel_points(WALL, first_index=1000 * f)
        if f < 2 and with_cluster:
            pts = np.concatenate([pts, voxel_points(CLUSTER, first_index=1000 * f + 500)])
        steps += [("insert", pts, f), ("carve", pts, SENSOR, f)]
    return LEAF, steps, both_radii(max_miss_ratio=1.0, min_neighbors=4) + both_radii(min_neighbors=4), dict(CARVE_PARAMS)


# ---- 5. the index edge --------------------------------------------------------------------------------------------------------
def index_edge():
    """per axis two layers of 3 x 3 voxels at the low end of the index range and two at the high end: a cell index that left the
    range and wrapped within the key would land in the other end's voxels, which are there to be found"""
    idx = []
    for axis in range(3):
        for layers in ([LO, LO + 1], [HI - 1, HI]):
            spans = [np.arange(-1, 2)] * 3
            spans[axis] = np.array(layers)
            idx.append(grid(*spans))
    idx = np.unique(np.concatenate(idx), axis=0)
    return LEAF, [("insert", voxel_points(idx), 0)], both_radii(min_neighbors=4), {}


def brute_force_neighbors(indices, r):
    idx = np.asarray(indices, np.int64)
    return (np.abs(idx[:, None, :] - idx[None, :, :]).max(axis=2) <= r).sum(axis=1)


def indices_of(voxels):
    k = voxels["key"]
    mask = np.uint64((1 << 21) - 1)
    return np.stack([k & mask, (k >> np.uint64(21)) & mask, k >> np.uint64(42)], axis=1).astype(np.int64) - DENSE_INDEX_RANGE


CASES = {"plane": plane, "row": row, "lone": lone, "plus": plus, "blocks": blocks, "oriented": oriented, "low_frames": low_frames,
         "seen_through": seen_through, "index_edge": index_edge}


# ---- 3. the oblique plane -----------------------------------------------------------------------------------------------------
OBLIQUE_NORMAL = np.array([0.3, -0.5, 0.81])
OBLIQUE_LEAF = 0.1


def oblique_plane(n=60000, sigma=0.01, seed=5, half=2.0):
    """n points of a square of side 2 * half on the plane through the origin with normal OBLIQUE_NORMAL, noise sigma along it"""
    rng = np.random.default_rng(seed)
    nrm = OBLIQUE_NORMAL / np.linalg.norm(OBLIQUE_NORMAL)
    u = np.cross(nrm, [0.0, 0.0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(nrm, u)
    ab = rng.uniform(-half, half, (n, 2))
    xyz = ab[:, :1] * u + ab[:, 1:] * v + rng.normal(0.0, sigma, (n, 1)) * nrm
    return cloud(xyz.astype(np.float32), intensity=rng.integers(0, 200, n))


# ---- clouds for the device's group and wavefront edges ------------------------------------------------------------------------
COUNTS = (1, 31, 32, 33, 63, 64, 65, 4097)


def counted(n):
    """n voxels packed in a cube, seen in frames 0 and 1, among twice as many seen in frame 0 alone: min_frames = 2 exports
    exactly n, sparser than the table"""
    pts = distinct_voxels(2 * n, seed=n)
    again = pts[:n].copy()
    again["time"] += 1.0
    return LEAF, [("insert", pts, 0), ("insert", again, 1)], both_radii(min_frames=2, viewpoints=[ABOVE]) + both_radii(), {}


# ---- playing a case -------------------------------------------------------------------------------------------------------------
def play(m, steps):
    """the steps into m, a DenseMapHost or a device DenseMap"""
    host = hasattr(m, "insert")
    for step in steps:
        if step[0] == "insert":
            (m.insert if host else m.insert_points)(step[1], step[2])
        elif host:
            m.carve(step[1], step[2], step[3], **CARVE_KW)
        else:
            m.carve_points(step[1], step[2], step[3])
    return m


def host_case(name):
    leaf, steps, queries, _ = CASES[name]()
    return play(DenseMapHost(leaf), steps), queries


def float_bits(normals):
    """(n, 4) uint32: the bits of the four floats"""
    n = np.ascontiguousarray(normals, dense_normal_dtype)
    return np.stack([n[f].view(np.uint32) for f in FLOATS], axis=1)


def no_normal(normals):
    """per record: are the four floats the NaN of "no normal" -- all four or none, anything else fails"""
    bits = float_bits(normals) == np.uint32(DENSE_NO_NORMAL)
    assert (bits.all(axis=1) | ~bits.any(axis=1)).all()
    assert not np.isnan(np.stack([normals[f] for f in FLOATS], axis=1)[~bits.all(axis=1)]).any()
    return bits.all(axis=1)
