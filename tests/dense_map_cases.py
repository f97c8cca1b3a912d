"""Cases for the dense point-cloud map (lidarslam_amd/_dense_map.py: DenseMapHost; lidarslam_amd/csrc/lsa_dense_map.hip).
Needs neither a GPU nor the native library.

Every coordinate is a multiple of 0.125 and the leaf is 0.5, as in tests/grid_cases.py: every quotient p / leaf is exact, and
points sit on voxel faces on purpose.  Points of a voxel may share coordinates; they differ in time and laser_id, so the
bytes of the map show which one was kept.

A case is a list of calls [(points, frame ordinal), ...].  In every case but `skipping` the host statement skips nothing
(`assert_nothing_skipped`), so that no case passes by leaving points out."""
import numpy as np

from lidarslam_amd._native import POINT_DTYPE

LEAF, STEP = 0.5, 0.125
SIZES = (0, 1, 63, 64, 65, 4096, 4097, 3 * 4096 + 1)  # distinct voxels of one call: wavefront, workgroup and 4096-point edges
RUNS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 4097)
BATCH = 3 * 4096 + 1


def cloud(xyz, intensity=None, first_index=0):
    """LidarPoints at xyz (n, 3) with w = 1; time and laser_id tell the points of a call apart"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    p = np.zeros(n, POINT_DTYPE)
    p["x"], p["y"], p["z"], p["w"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1.0
    i = np.arange(first_index, first_index + n)
    p["time"] = -0.1 + 1e-6 * i
    p["intensity"] = (i % 251).astype(np.float32) if intensity is None else np.asarray(intensity, np.float32)
    p["laser_id"] = i % 128
    p["label"] = i % 3
    return p


def voxel_corners(n, seed=0):
    """n distinct voxel indices (n, 3) around the origin, negative ones among them"""
    rng = np.random.default_rng(seed)
    side = max(int(np.ceil(n ** (1 / 3))) + 2, 4)
    flat = rng.permutation(side**3)[:n]
    idx = np.stack([flat % side, (flat // side) % side, flat // (side * side)], axis=1) - side // 2
    return idx


def distinct_voxels(n, seed=0):
    """one point in each of n distinct voxels, at one of the 4^3 lattice places of the voxel (its lower faces among them)"""
    rng = np.random.default_rng(seed + 17)
    idx = voxel_corners(n, seed)
    inside = rng.integers(0, 4, size=(n, 3)) * STEP
    return cloud(idx * LEAF + inside, intensity=rng.integers(0, 200, n))


def one_voxel(n, intensity=7.0):
    """n points of one voxel with equal intensities: the smallest index of the call wins"""
    rng = np.random.default_rng(3)
    return cloud(np.array([-1.0, 2.0, -3.5]) + rng.integers(0, 4, size=(n, 3)) * STEP, intensity=np.full(n, intensity))


def runs(order):
    """BATCH points in runs of RUNS points a voxel, the rest one a voxel; intensities from a small set so that every long
    run has ties.  order: 'contiguous', 'interleaved' (a fixed shuffle) or 'reversed'"""
    lengths = list(RUNS) + [1] * (BATCH - sum(RUNS))
    idx = voxel_corners(len(lengths), seed=5)
    rng = np.random.default_rng(11)
    xyz = np.concatenate([idx[v] * LEAF + rng.integers(0, 4, size=(length, 3)) * STEP for v, length in enumerate(lengths)])
    inten = rng.integers(0, 5, xyz.shape[0]).astype(np.float32)
    perm = {"contiguous": np.arange(BATCH), "interleaved": np.random.default_rng(23).permutation(BATCH), "reversed": np.arange(BATCH)[::-1]}[order]
    return cloud(xyz[perm], intensity=inten[perm])


def growth_calls():
    """12 289 distinct voxels over 5 calls; calls 2 and 4 also revisit voxels of the calls before them"""
    first = distinct_voxels(BATCH, seed=9)
    cuts = [0, 40, 1000, 3000, 7000, BATCH]
    calls = []
    for c in range(5):
        part = first[cuts[c]:cuts[c + 1]]
        if c in (2, 4):
            again = first[: cuts[c] : 3].copy()
            again["intensity"] += np.float32(c)  # some now win their voxel, some do not
            again["time"] += 1.0
            part = np.concatenate([again, part])
        calls.append((part, c))
    return calls


def stress_calls():
    """2 048 keys at most, over three calls that revisit: with "ProbeStress" every probe sequence starts at slot 0"""
    a = distinct_voxels(2048, seed=4)
    b = a[::2].copy()
    b["intensity"] += 3
    return [(a[:1500], 0), (b, 1), (a[1500:], 1)]


# ---- the properties of the definition: (calls, what the map must be) ---------------------------------------------------------
def negative_coordinates():
    """-0.0 falls into voxel 0, -0.125 into voxel -1; floor, not truncation"""
    xyz = [[-0.0, 0.0, 0.0], [-0.125, 0.0, 0.0], [0.375, -0.5, 0.0], [-0.5, -0.625, -1.0], [0.0, 0.0, -0.0]]
    return [(cloud(xyz, intensity=[1, 2, 3, 4, 5]), 0)], [(0, 0, 0), (-1, 0, 0), (0, -1, 0), (-1, -2, -2), (0, 0, 0)]


def faces():
    """points exactly on faces belong to the voxel above; the last lattice place below a face to the one below"""
    xyz = [[0.5, 0.0, 0.0], [0.375, 0.0, 0.0], [1.0, 1.0, 1.0], [0.875, 0.875, 0.875], [-0.5, -0.5, -0.5], [-0.625, -0.5, -0.5], [0.0, 0.5, -0.5]]
    return [(cloud(xyz), 0)], [(1, 0, 0), (0, 0, 0), (2, 2, 2), (1, 1, 1), (-1, -1, -1), (-2, -1, -1), (0, 1, -1)]


def ties():
    """within a call the lowest index of the largest intensity wins; across calls the earlier frame keeps a tie"""
    a = cloud([[0.125, 0.125, 0.125]] * 4 + [[2.0, 0.0, 0.0]], intensity=[3, 9, 9, 1, 4])
    b = cloud([[0.25, 0.25, 0.25]] * 3 + [[2.125, 0.0, 0.0]], intensity=[9, 2, 9, 5], first_index=100)
    return [(a, 0), (b, 1)]


def nan_intensity():
    """a NaN intensity loses to every number, -inf among them; a voxel of NaNs alone keeps its lowest index, and any number
    of a later frame replaces it"""
    a = cloud([[0.0, 0.0, 0.0]] * 3 + [[1.0, 0.0, 0.0]] * 2 + [[2.0, 0.0, 0.0]], intensity=[np.nan, -np.inf, np.nan, np.nan, np.nan, 5.0])
    b = cloud([[1.125, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0]], intensity=[-1e30, np.nan, np.nan], first_index=50)
    return [(a, 0), (b, 3)]


def signed_zero():
    """intensities are compared by their ordered code, under which -0.0 ranks below +0.0: +0.0 wins a voxel over an earlier
    -0.0 of the same call and replaces a -0.0 of an earlier frame; a -0.0 replaces neither"""
    a = cloud([[0.0, 0.0, 0.0]] * 2 + [[1.0, 0.0, 0.0]] + [[2.0, 0.0, 0.0]], intensity=[-0.0, 0.0, -0.0, 0.0])
    b = cloud([[1.125, 0.0, 0.0], [2.125, 0.0, 0.0], [0.125, 0.0, 0.0]], intensity=[0.0, -0.0, -0.0], first_index=30)
    return [(a, 0), (b, 1)]


def skipping():
    """non-finite coordinates and indices outside [-2^20, 2^20) take no part: 7 of the 10 points"""
    edge = float(1 << 20) * LEAF
    xyz = [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [edge, 0, 0], [0, -edge - STEP, 0], [3e38, 0, 0], [0, 0, edge + 4.0],
           [edge - STEP, 0, 0], [0, -edge, 0], [0.125, 0.125, 0.125]]
    return [(cloud(xyz), 0)], 7, [((1 << 20) - 1, 0, 0), (0, -(1 << 20), 0), (0, 0, 0)]


def same_ordinal_twice():
    """two calls with one ordinal (two LiDAR devices of one AddFrames call) count one frame; the count still adds up"""
    a = cloud([[0.0, 0.0, 0.0]] * 2 + [[1.0, 0.0, 0.0]], intensity=[1, 2, 3])
    b = cloud([[0.125, 0.0, 0.0], [3.0, 0.0, 0.0]], intensity=[5, 1], first_index=10)
    c = cloud([[0.25, 0.0, 0.0]], intensity=[0], first_index=20)
    return [(a, 4), (b, 4), (c, 6)]


def wall_and_mover(frames=8):
    """a wall of 9 x 9 voxels seen in every frame and a cluster that moves one voxel a frame: get(3) is the wall alone"""
    g = np.arange(-4, 5)
    wall = np.stack(np.meshgrid([6], g, g, indexing="ij"), axis=-1).reshape(-1, 3) * LEAF + STEP
    calls = []
    for f in range(frames):
        mover = np.array([[f - 3, 0, 0]]) * LEAF + np.array([[0, 0, 0], [STEP, STEP, 0], [2 * STEP, 0, STEP]])
        calls.append((cloud(np.concatenate([wall, mover]), first_index=1000 * f), f))
    return calls, wall.shape[0]


PROPERTY_CASES = {
    "negative": lambda: negative_coordinates()[0], "faces": lambda: faces()[0], "ties": ties, "nan": nan_intensity,
    "skipping": lambda: skipping()[0], "ordinal": same_ordinal_twice, "signed_zero": signed_zero, "wall": lambda: wall_and_mover()[0],
}


def key_of(index):
    ix, iy, iz = (int(v) + (1 << 20) for v in index)
    return (iz << 42) | (iy << 21) | ix


def host_map(DenseMapHost, calls, leaf=LEAF):
    h = DenseMapHost(leaf)
    for pts, frame in calls:
        h.insert(pts, frame)
    return h


def assert_nothing_skipped(DenseMapHost, calls, leaf=LEAF):
    h = host_map(DenseMapHost, calls, leaf)
    assert h.skipped == 0
    return h
