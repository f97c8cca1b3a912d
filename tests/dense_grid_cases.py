"""Cases for the dense map's floor plan (lidarslam_amd/_dense_map.py: DenseMapHost.grid, dense_grid;
lidarslam_amd/csrc/lsa_dense_grid.hip: k_dense_grid_*).  Needs neither a GPU nor the native library.

A case is (leaf, steps, queries, device parameters): `steps` build the map as in tests/dense_normals_cases.py and every query
is a dict of keyword arguments of grid().  The host tests (tests/test_dense_grid_host.py) assert, by hand, what the definition
must give; the GPU tests (tests/test_gpu_dense_grid.py) hold the device to the host statement on every case and query, byte
for byte.

The leaf is 0.25 and points sit at voxel centres unless a case says otherwise, so that every z, and every height above the
ground, is exact: voxel iz has z = 0.25 * iz + 0.125."""
import numpy as np

from dense_map_cases import cloud
from dense_normals_cases import CARVE_PARAMS, play  # noqa: F401 (play: used by the tests)
from lidarslam_amd._dense_map import DENSE_GRID_ABSENT, DENSE_INDEX_RANGE, DenseMapHost, dense_cell_dtype

LEAF = 0.25
F32 = np.float32
FLOATS = ("elevation", "ground", "top")


def Z(iz):
    """the z of the centre of voxel iz"""
    return float(F32(LEAF * iz + LEAF / 2))


def box(xs, ys, zs):
    return np.stack(np.meshgrid(xs, ys, zs, indexing="ij"), axis=-1).reshape(-1, 3)


def at(indices, z=None, first_index=0, leaf=LEAF):
    """one LidarPoint at the centre of every voxel index (n, 3); z: the points' z instead of the centres'"""
    idx = np.asarray(indices, np.float64).reshape(-1, 3)
    xyz = (idx + 0.5) * leaf
    if z is not None:
        xyz[:, 2] = np.asarray(z, np.float64)
    p = cloud(xyz, first_index=first_index)
    if z is not None:
        p["z"] = np.asarray(z, F32)  # the bits asked for: a -0.0, one ulp above a number
    return p


# ---- the scenes of the definition (cell_leaves = 1 unless the query says otherwise: a cell is a voxel column) -------------------
def wall():
    """a floor of 6 x 3 cells whose cells under the wall (x = 3) were never seen, and the wall, voxels iz 2..5, above them"""
    floor = box([0, 1, 2, 4, 5], [0, 1, 2], [0])
    bricks = box([3], [0, 1, 2], [2, 3, 4, 5])
    return LEAF, [("insert", at(np.concatenate([floor, bricks])), 0)], [dict(cell_leaves=1), dict(cell_leaves=1, ground_radius=0)], {}


def pole():
    """a floor of 5 x 5 cells, a pole of six voxels on cell (2, 2) and a stub of one voxel on cell (0, 0)"""
    idx = np.concatenate([box(range(5), range(5), [0]), box([2], [2], range(1, 7)), box([0], [0], [2])])
    return LEAF, [("insert", at(idx), 0)], [dict(cell_leaves=1), dict(cell_leaves=1, min_obstacle_voxels=2), dict(cell_leaves=1, min_obstacle_voxels=7)], {}


def slab():
    """a slab at iz 10 (2.5 above the floor: over max_height 2) over cells x 0..2 whose floor was seen at x = 0 alone, and,
    far from any floor (x 8, 9), a slab that is its own ground"""
    idx = np.concatenate([box([0], range(3), [0]), box([0, 1, 2, 8, 9], range(3), [10])])
    return LEAF, [("insert", at(idx), 0)], [dict(cell_leaves=1), dict(cell_leaves=1, max_height=2.5), dict(cell_leaves=1, max_height=float(np.nextafter(2.5, 0)))], {}


KERB_MIN = 0.25
KERB_UP = float(np.nextafter(F32(Z(1)), F32(9)))  # one float above the kerb of exactly min_height


def kerb():
    """a floor row x 0..3 at z = 0.125; on cell 1 a kerb whose point lies exactly min_height = 0.25 above it, on cell 2 one a
    single float higher"""
    floor = at(box(range(4), [0], [0]))
    kerbs = at([[1, 0, 1], [2, 0, 1]], z=[Z(1), KERB_UP], first_index=50)
    return LEAF, [("insert", np.concatenate([floor, kerbs]), 0)], [dict(cell_leaves=1, min_height=KERB_MIN), dict(cell_leaves=1, min_height=KERB_MIN, ground_radius=0)], {}


RAMP_STEP = 0.0625  # a cell: 25 %


def ramp(step=RAMP_STEP, n=12):
    """a row of n cells, each `step` higher than the one before it; the points lie on the ramp, not at the centres"""
    z = F32(0.03125) + F32(step) * np.arange(n, dtype=F32)
    idx = np.stack([np.arange(n), np.zeros(n), np.floor(z.astype(np.float64) / LEAF)], axis=1)
    return LEAF, [("insert", at(idx, z=z), 0)], [dict(cell_leaves=1), dict(cell_leaves=1, ground_radius=4), dict(cell_leaves=1, ground_radius=0)], {}


CAR_SENSOR = np.array([[0.125, 0.125, Z(2)]], F32)


def car():
    """a floor of 9 x 3 cells and a back wall voxel (8, 0, 2) seen in six frames; a car voxel (4, 0, 2) hit in frame 0 alone and
    seen through, on the way to the wall, in frames 1..5: misses 5 > 1 * frames"""
    floor, back, vehicle = box(range(9), [-1, 0, 1], [0]), [[8, 0, 2]], [[4, 0, 2]]
    steps = []
    for f in range(6):
        pts = at(np.concatenate([floor, back] + ([vehicle] if f == 0 else [])), first_index=100 * f)
        steps += [("insert", pts, f), ("carve", at(back), CAR_SENSOR, f)]
    return LEAF, steps, [dict(cell_leaves=1, max_miss_ratio=1.0), dict(cell_leaves=1), dict(cell_leaves=1, min_frames=2)], dict(CARVE_PARAMS)


def both_sides():
    """a floor of 8 x 2 voxels, ix -4..3, iy -1..0: with floor division voxel -1 is in cell -1 for every cell_leaves"""
    return LEAF, [("insert", at(box(range(-4, 4), [-1, 0], [0])), 0)], [dict(cell_leaves=c, ground_radius=1) for c in (1, 2, 3)], {}


def signed_zero():
    """one cell (cell_leaves 2) of two voxels whose points have z = +0.0 and z = -0.0: the elevation is -0.0"""
    pts = at([[0, 0, 0], [1, 0, 0]], z=[0.0, -0.0])
    return LEAF, [("insert", pts, 0)], [dict(cell_leaves=2)], {}


def signed_zero_top():
    """the same pair one metre above a floor voxel of the cell: both are obstacles, the top is +0.0"""
    pts = at([[0, 0, 0], [1, 0, 0], [0, 1, -4]], z=[0.0, -0.0, -1.0])
    return LEAF, [("insert", pts, 0)], [dict(cell_leaves=2)], {}


def radius():
    """a floor voxel in cell 0 and voxels one metre higher in cells 16 and 17: the ground of cell 0 reaches cell 16 under
    ground_radius 16 and never cell 17"""
    return LEAF, [("insert", at([[0, 0, 0], [16, 0, 4], [17, 0, 4]]), 0)], [dict(cell_leaves=1, ground_radius=g) for g in (16, 0, 15)], {}


def one_cell():
    return LEAF, [("insert", at([[-3, 5, 1]]), 0)], [dict(cell_leaves=c, ground_radius=g) for c in (1, 2, 64) for g in (0, 16)], {}


WIDTHS = (1, 63, 64, 65)


def wide(n):
    """a floor of n x 3 cells (cell_leaves 2: 2n x 6 voxels) from x cell -n // 2 on, a post on every seventh cell"""
    x0 = -(n // 2) * 2
    floor = box(range(x0, x0 + 2 * n), range(6), [0])
    posts = box(range(x0, x0 + 2 * n, 14), [2], [1, 2, 3])
    return LEAF, [("insert", at(np.concatenate([floor, posts])), 0)], [dict(), dict(ground_radius=0), dict(cell_leaves=1, ground_radius=16)], {}


def scattered(seed=3, n=3000, leaf=0.125):
    """n points of a rough scene: a floor with holes, boxes and poles on it, things above max_height -- off the lattice, both
    sides of 0, several points a voxel"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-4.0, 4.0, (n, 2))
    kind = rng.integers(0, 10, n)
    xy = np.where((kind >= 6)[:, None], np.floor(xy) + 0.3 * (xy - np.floor(xy)), xy)  # what stands on the floor stands in clusters
    z = np.where(kind < 6, rng.normal(0.0, 0.02, n) + 0.05 * xy[:, 0], np.where(kind < 9, rng.uniform(0.0, 1.8, n), rng.uniform(2.0, 4.0, n)))
    keep = ~((np.abs(xy[:, 0] - 1.0) < 0.7) & (np.abs(xy[:, 1] + 1.0) < 0.7) & (kind < 6))  # a hole in the floor
    xyz = np.concatenate([xy, z[:, None]], axis=1)[keep]
    return leaf, cloud(xyz.astype(F32), intensity=rng.integers(0, 200, xyz.shape[0]))


SCATTERED_QUERIES = [dict(), dict(cell_leaves=1, ground_radius=3), dict(cell_leaves=3, ground_radius=1, min_obstacle_voxels=2), dict(cell_leaves=5, ground_radius=16, min_height=0.1, max_height=1.0)]
# windows (x_min, y_min, x_max, y_max) against the scattered scene, which spans [-4, 4]^2: inside it, across its edge, outside
# it, a single point, and all of it with a margin
WINDOWS = {"inside": (-1.3, -2.2, 2.6, 1.1), "across": (2.0, -6.0, 7.5, 0.3), "outside": (9.0, 9.0, 11.0, 12.5), "point": (0.3, 0.3, 0.3, 0.3), "around": (-8.0, -8.0, 8.0, 8.0)}


def scattered_case():
    leaf, pts = scattered()
    half = len(pts) // 2
    queries = list(SCATTERED_QUERIES) + [dict(q, window=w) for q in SCATTERED_QUERIES[:3] for w in WINDOWS.values()]
    return leaf, [("insert", pts[:half], 0), ("insert", pts[half:], 1)], queries, {}


CASES = {"wall": wall, "pole": pole, "slab": slab, "kerb": kerb, "ramp": ramp, "car": car, "both_sides": both_sides, "signed_zero": signed_zero,
         "signed_zero_top": signed_zero_top, "radius": radius, "one_cell": one_cell, "scattered": scattered_case}
CASES.update({f"wide{n}": (lambda n=n: wide(n)) for n in WIDTHS})


def host_case(name):
    leaf, steps, queries, _ = CASES[name]()
    return play(DenseMapHost(leaf), steps), queries


# ---- comparing grids ---------------------------------------------------------------------------------------------------------------
def float_bits(cells):
    """(..., 3) uint32: the bits of elevation, ground, top"""
    c = np.ascontiguousarray(cells, dense_cell_dtype)
    return np.stack([c[f].view(np.uint32) for f in FLOATS], axis=-1)


def absent(cells, field):
    return np.ascontiguousarray(cells[field]).view(np.uint32) == np.uint32(DENSE_GRID_ABSENT)


def same_grid(got, want):
    """info, all 20 bytes of every record and every state are equal; returns the number of cells"""
    (gi, gc, gs), (wi, wc, ws) = got, want
    assert gi.tobytes() == wi.tobytes(), (gi, wi)
    assert gc.dtype == wc.dtype and gc.dtype.itemsize == 20 and gc.shape == wc.shape == gs.shape == ws.shape == (int(wi["height"]), int(wi["width"]))
    assert gs.dtype == ws.dtype == np.int8 and gs.tobytes() == ws.tobytes(), int((gs != ws).sum())
    assert gc.tobytes() == wc.tobytes(), {f: int((np.ascontiguousarray(gc[f]).view(np.uint32) != np.ascontiguousarray(wc[f]).view(np.uint32)).sum()) for f in gc.dtype.names}
    return gs.size


def crop(whole, info):
    """(cells, state) of the extent of `info` cut out of the grid `whole`, whose extent must contain it"""
    wi, wc, ws = whole
    x, y = int(info["cx0"]) - int(wi["cx0"]), int(info["cy0"]) - int(wi["cy0"])
    w, h = int(info["width"]), int(info["height"])
    assert 0 <= x and 0 <= y and x + w <= int(wi["width"]) and y + h <= int(wi["height"])
    return wc[y:y + h, x:x + w], ws[y:y + h, x:x + w]


def far_apart():
    """two voxels 2^20 leaves apart in x and in y: a whole grid of (2^19 + 1)^2 cells at cell_leaves 2"""
    return at([[-(DENSE_INDEX_RANGE // 2), -(DENSE_INDEX_RANGE // 2), 0], [DENSE_INDEX_RANGE // 2, DENSE_INDEX_RANGE // 2, 0]])
