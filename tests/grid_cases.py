"""Cases for the rolling voxel map (RollingGrid::Add, Roll, BuildSubMapKdTree) at the shapes the device map's kernels branch
on (lsa_grid_add.hip, lsa_device_grid.hip, lsa_grid_submap.hip), and a plain statement of the per-voxel rule to hold the
oracle to.  Needs neither a GPU nor the native library.

The statement.  `voxel_keys` is Utils::PositionToVoxel (RollingGrid.h:39-42) applied twice in float32 -- round half away
from zero --, To1d of the outer and of the (possibly negative) leaf coordinates and the inside test, as RollingGrid.cxx:177-202
has them.  `fold_statement` is the rule of :203-311 for the samplings FIRST, LAST, MAX_INTENSITY and CENTER_POINT: a walk over
the points in arrival order with a dictionary per key.  `roll_offset` is :122-130.  CENTROID has no closed form (the pulls of
:282-297 couple the voxels); the oracle alone is its reference.

One thing the statement makes plain: the "centre" CENTER_POINT measures to (:257) is voxelGridCenterIn - VoxelResolution / 2
+ LeafSize * voxelCoordIn with leaf coordinates that run from -4 to 4 around the outer voxel's centre -- half an outer voxel
below the leaf's true centre on every axis.  Points "mirrored about the centre" are therefore mirrored in the plane y = z
through that point (the y and z offsets swapped): both lie in the same leaf, and x^2 + (y^2 + z^2) is the same sum.

The cases.  Every coordinate is a multiple of 0.125, LeafSize 0.5, VoxelResolution 4.0: every quotient of the key and every
square of CENTER_POINT is exact in float32.  GridSize 6 and 7 (even and odd; both at most 8, so the nine leaf coordinates
-4..4 of an axis alias in To1d: one key, two leaves, two centres) and 12 (no aliasing).  Points of a voxel may share
coordinates; they differ in time, intensity and laser_id, so the bytes of the map show which one was kept.

  1. run structure: 3 * 4096 + 1 points over a few hundred voxels, runs of 1, 2, 255, 256, 257, 513 and 4097 points among
     them, 391 points outside the grid, in three arrival orders -- every run contiguous; interleaved (point i of a run of L at
     the fraction (i + 0.5) / L of the batch, so every run is spread evenly over the sort runs; the fourth sort run holds ONE
     point, which is the longest run's); reversed -- and 1, 255, 256, 257 points in one voxel.  Each is added twice,
     the second time partly onto other voxels.
  2. ties and rules: intensity patterns, equal distances, a second Add onto long runs, fixed voxels, Adds that change nothing.
  3. faces: points on leaf, outer and grid faces; rolls by exactly +-0.5 and +-1.5 outer voxels; sub-map boxes on faces,
     outside the grid and in the wrong order.
  4. several maps in one launch (`MultiCase`).

Layers 1 and 2 run with MinFramesPerVoxel 1 (2 in `second_add`): a later Add hits only some of the voxels, so the clean map
(count > MinFramesPerVoxel) is a proper part of the map and a voxel counted twice in one Add, or not at all, shows in it.

Dropped as undefined: a batch with NaN points.  The reference casts round(NaN) to int (PositionToVoxel), which C++ leaves
undefined, and takes the box with pcl::getMinMax3D, whose Eigen min / max on a cloud flagged dense do not say which operand a
NaN comparison keeps.  The oracle picks one answer for each; the reference promises neither.

`vacuity_problems(case)` lists what a case is there to contain and does not; it uses the keys and a sort only."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from lidarslam_amd._native import POINT_DTYPE

f32 = np.float32
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
LEAF, RES, STEP = 0.5, 4.0, 0.125
BLOCK, SORT_RUN = 256, 4096  # places per block of the fold, pairs per run of the sort
BATCH = 3 * SORT_RUN + 1
RUNS = (1, 2, 255, 256, 257, 513, 4097)
TAIL = 391
GRID_SIZES = (6, 7, 12)


# ---- the statement ----------------------------------------------------------------------------------------------------------
def round_half_away(v):
    """std::round of a float array (as floats)"""
    a = np.abs(v)
    f = np.floor(a)
    f = f + (a - f >= 0.5)
    return np.where(v < 0, -f, f)


def position_to_voxel(p, origin, resolution):
    """((p - origin) / resolution).round().cast<int>() in float32; what does not fit an int (or is NaN) becomes INT_MIN"""
    r = round_half_away((p.astype(f32) - origin.astype(f32)) / f32(resolution))
    ok = (r >= -2147483648.0) & (r < 2147483648.0)
    return np.where(ok, r, -2147483648.0).astype(np.int64)


def grid_origin(grid_size, resolution, position):
    """voxelGridOrigin = VoxelGridPosition - int(GridSize / 2) * VoxelResolution (:177): the centre of outer voxel (0, 0, 0)"""
    return np.asarray(position, f32) - f32(int(grid_size / 2) * float(resolution))


def voxel_coords(xyz, grid_size, resolution, leaf, position):
    """outer coordinates, leaf coordinates, inside, centre of the outer voxel -- of every point (:191-200)"""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    origin = grid_origin(grid_size, resolution, position)
    out = position_to_voxel(xyz, origin, resolution)
    inside = np.all((out >= 0) & (out < grid_size), axis=1)
    centre = np.where(inside[:, None], out, 0).astype(f32) * f32(resolution) + origin
    inn = position_to_voxel(xyz, centre, leaf)
    return out, inn, inside, centre


def voxel_keys(xyz, grid_size, resolution, leaf, position):
    """(To1d(outer) << 32) | unsigned(To1d(leaf)) per point, NO_KEY outside the grid: the order of the map is the order of
    these numbers"""
    out, inn, inside, _ = voxel_coords(xyz, grid_size, resolution, leaf, position)
    g = int(grid_size)
    out = np.where(inside[:, None], out, 0)
    inn = np.where(inside[:, None], inn, 0)
    idx_out = out[:, 2] * g * g + out[:, 1] * g + out[:, 0]
    idx_in = (inn[:, 2] * g * g + inn[:, 1] * g + inn[:, 0]) & 0xFFFFFFFF
    key = (idx_out.astype(np.uint64) << np.uint64(32)) | idx_in.astype(np.uint64)
    return np.where(inside, key, NO_KEY)


def xyz_of(points):
    return np.stack([points["x"], points["y"], points["z"]], 1).astype(f32)


def norm3(d):
    """Eigen's Vector3f::norm: sqrt(x^2 + (y^2 + z^2)) in float32"""
    d = np.asarray(d, f32)
    return np.sqrt(d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))


def leaf_centres(xyz, grid_size, resolution, leaf, position):
    """the point CENTER_POINT measures to, for the leaf of every point (:257)"""
    _, inn, _, centre = voxel_coords(xyz, grid_size, resolution, leaf, position)
    return (centre - f32(float(resolution) / 2.0)) + f32(leaf) * inn.astype(f32)


def fold_statement(points, sampling, time, fixed, previous=None, *, grid_size, resolution=RES, leaf=LEAF, position=(0.0, 0.0, 0.0)):
    """The map one Add(points, fixed, time, roll=False) leaves, as (keys, points, counts) in key order; `previous` is such a
    triple.  Samplings 0-3."""
    assert sampling in (0, 1, 2, 3)
    points = np.ascontiguousarray(points, POINT_DTYPE)
    if previous is None:
        previous = (np.zeros(0, np.uint64), np.zeros(0, POINT_DTYPE), np.zeros(0, np.uint32))
    pk, pp, pc = previous
    if points.size == 0:
        return pk.copy(), pp.copy(), pc.copy()  # "Pointcloud is empty, voxel grid not updated." (:162-166)
    xyz = xyz_of(points)
    keys = voxel_keys(xyz, grid_size, resolution, leaf, position)
    P = pp.size
    pool = np.concatenate([pp, points])
    pool_xyz = xyz_of(pool)
    intensity = pool["intensity"].tolist()
    src = {int(k): j for j, k in enumerate(pk)}       # key -> which point of the pool the voxel holds
    cnt = {int(k): int(c) for k, c in zip(pk, pc)}
    lab = {int(k): int(l) for k, l in zip(pk, pp["label"])}
    if sampling == 3:
        centres = leaf_centres(xyz, grid_size, resolution, leaf, position)
        own = norm3(xyz - centres).tolist()
    seen = set()
    label = 1 if fixed else 0
    no_key = int(NO_KEY)
    for i, k in enumerate(keys.tolist()):
        if k == no_key:
            continue
        if k not in src:
            src[k] = P + i  # first arrival (:204-211)
            cnt[k] = 0
        else:
            if lab[k] == 1:
                continue  # a voxel whose point is fixed takes nothing, not even the time (:218-219)
            if sampling == 1:
                src[k] = P + i
            elif sampling == 2:
                if intensity[P + i] > intensity[src[k]]:
                    src[k] = P + i
            elif sampling == 3:
                if own[i] < float(norm3(pool_xyz[src[k]] - centres[i])):
                    src[k] = P + i
        lab[k] = label
        if k not in seen:
            cnt[k] += 1  # one count per call (:307-311)
            seen.add(k)
    order = sorted(src)
    out = pool[[src[k] for k in order]]
    stamped = np.array([k in seen for k in order], bool)
    out["time"][stamped] = time
    out["label"][stamped] = label
    return np.array(order, np.uint64), out, np.array([cnt[k] for k in order], np.uint32)


def roll_offset(mn, mx, grid_size, resolution, position):
    """Roll (:122-130): the clamped offset over the resolution per axis, and the outer voxels the grid moves by"""
    mn, mx, pos = np.asarray(mn, f32), np.asarray(mx, f32), np.asarray(position, f32)
    h = f32(float(grid_size) / 2 * float(resolution))
    down, up = mn - (pos - h), mx - (pos + h)
    off = (up + down) / f32(2)
    off = np.minimum(np.maximum(off, np.minimum(down, f32(0))), np.maximum(up, f32(0)))
    q = off / f32(resolution)
    return q, round_half_away(q).astype(np.int64), (down, up)


def box_of(points):
    """pcl::getMinMax3D of a cloud without NaN"""
    xyz = xyz_of(points)
    return xyz.min(axis=0), xyz.max(axis=0)


class Statement:
    """Add / Roll / Get / Size of one map by the statement (samplings 0-3; nothing decays, so Size is the number of voxels)"""

    def __init__(self, grid_size, sampling, min_frames=0, resolution=RES, leaf=LEAF):
        self.g, self.res, self.leaf, self.sampling, self.min_frames = int(grid_size), resolution, leaf, sampling, min_frames
        self.position = np.zeros(3, f32)
        self.map = (np.zeros(0, np.uint64), np.zeros(0, POINT_DTYPE), np.zeros(0, np.uint32))

    def roll(self, mn, mx):
        _, vox, _ = roll_offset(mn, mx, self.g, self.res, self.position)
        if not vox.any():
            return
        keys, pts, cnt = self.map
        g = self.g
        idx = (keys >> np.uint64(32)).astype(np.int64)
        z, y, x = idx // (g * g), (idx // g) % g, idx % g
        x, y, z = x - vox[0], y - vox[1], z - vox[2]
        keep = (x >= 0) & (x < g) & (y >= 0) & (y < g) & (z >= 0) & (z < g)
        new = ((z * g * g + y * g + x).astype(np.uint64) << np.uint64(32)) | (keys & np.uint64(0xFFFFFFFF))
        new, pts, cnt = new[keep], pts[keep], cnt[keep]
        o = np.argsort(new, kind="stable")
        self.map = (new[o], pts[o], cnt[o])
        self.position = self.position + vox.astype(f32) * f32(self.res)

    def add(self, points, fixed=False, time=-1.0, roll=True):
        if points.size == 0:
            return
        if roll:
            self.roll(*box_of(points))
        self.map = fold_statement(points, self.sampling, time, fixed, self.map, grid_size=self.g, resolution=self.res, leaf=self.leaf, position=self.position)

    def size(self):
        return self.map[0].size

    def get(self, clean=False):
        return self.map[1][self.map[2] > self.min_frames] if clean else self.map[1].copy()


# ---- cases ------------------------------------------------------------------------------------------------------------------
@dataclass
class Add:
    points: np.ndarray
    fixed: bool = False
    time: float = -1.0
    roll: bool = False
    still_valid: tuple = ()  # samplings under which the Add changes no point: the sub-map built before stays valid


@dataclass
class Roll:
    mn: np.ndarray
    mx: np.ndarray


@dataclass
class SubMap:
    mn: np.ndarray
    mx: np.ndarray
    min_nb: int


@dataclass
class Case:
    name: str
    layer: int
    grid_size: int
    ops: list
    wants: tuple            # what vacuity_problems holds the case to
    min_frames: int = 0
    sampling: int = None    # None: every sampling
    centroid: bool = False  # few enough voxels for the oracle's CENTROID loop (points x voxels)

    def params(self):
        return dict(GridSize=self.grid_size, LeafSize=LEAF, VoxelResolution=RES, MinFramesPerVoxel=self.min_frames)

    def samplings(self):
        return (0, 1, 2, 3) if self.sampling is None else (self.sampling,)


def play(case, sampling, g, o, same_state, same_submap):
    """the case's calls on both maps (made with `sampling`); after every modification the state, the validity of the sub-map
    built before it, and the whole map as a sub-map"""
    for op in case.ops:
        if isinstance(op, SubMap):
            n = same_submap(g, o, op.mn, op.mx, op.min_nb)
            if np.any(op.mn > op.mx):
                assert n == 0 and not o.submap_valid()
            continue
        if isinstance(op, Add):
            for m in (g, o):
                m.add(op.points, fixed=op.fixed, time=op.time, roll=op.roll)
        else:
            for m in (g, o):
                m.roll(op.mn, op.mx)
        same_state(g, o)
        assert g.submap_valid() == o.submap_valid()
        if isinstance(op, Add) and sampling in op.still_valid:
            assert o.submap_valid()  # nothing changed: RollingGrid.cxx:315-317 keeps the kd-tree
        same_submap(g, o)


def make_points(xyz, rng, t0=0.0, levels=4):
    """points at xyz (float64 multiples of 0.125, exact in float32) in this arrival order: integer intensities that tie, time
    and laser_id that tell every point from every other"""
    n = len(xyz)
    p = np.zeros(n, POINT_DTYPE)
    xyz = np.asarray(xyz, np.float64).reshape(n, 3)
    assert np.all(xyz * 8 == np.round(xyz * 8))
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    p["intensity"] = rng.integers(0, levels, n).astype(f32)
    p["time"] = t0 + np.arange(n) * 1e-5
    p["laser_id"] = np.arange(n) % 65536
    return p


def origin_of(g):
    return -float(int(g / 2)) * RES


def lattice_pool(g):
    """lattice points of a few outer voxels: 32 x 32 steps of 0.125 in x and y around the centre, a few layers in z -- the
    lowest step of an axis lies ON the outer face (and, in outer voxel 0, on the grid's own face: outside)"""
    outers = [(0, 0, 0), (g - 1, g - 1, g - 1), (1, 0, g - 1), (g // 2, g // 2, g // 2), (g // 2 - 1, g - 1, 1), (g - 1, 1, 0),
              (2, 3, 2), (0, g - 1, g // 2), (3, 1, 4), (1, 2, 1), (g - 2, g - 2, 0), (4, 4, g - 1)]
    m = np.arange(-16, 16)
    mx, my, mzz = np.meshgrid(m, m, np.array([-16, -3, 0, 2, 15]), indexing="ij")
    local = np.stack([mx.ravel(), my.ravel(), mzz.ravel()], 1) * STEP
    return np.concatenate([origin_of(g) + RES * np.array(o, np.float64) + local for o in outers])


def leaf_ids(inn):
    """one number per leaf of an outer voxel (unlike To1d, which lets leaves alias)"""
    return (inn[:, 2] + 8) * 400 + (inn[:, 1] + 8) * 20 + (inn[:, 0] + 8)


def keyed_pool(g):
    """the pool's points inside the grid, grouped by key: (xyz, list of index arrays, one per key in key order, aliased flags)"""
    xyz, groups, aliased = _keyed_pool(g)
    return xyz, list(groups), aliased


@lru_cache(maxsize=None)
def _keyed_pool(g):
    xyz = lattice_pool(g)
    keys = voxel_keys(xyz, g, RES, LEAF, (0, 0, 0))
    xyz, keys = xyz[keys != NO_KEY], keys[keys != NO_KEY]
    _, inn, _, _ = voxel_coords(xyz, g, RES, LEAF, (0, 0, 0))
    leaf_id = leaf_ids(inn)
    order = np.lexsort((leaf_id, keys))
    xyz, keys, leaf_id = xyz[order], keys[order], leaf_id[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    groups = np.split(np.arange(keys.size), starts[1:])
    aliased = np.array([leaf_id[grp[0]] != leaf_id[grp[-1]] for grp in groups])
    # a group's members alternate between its leaves, so that even a run of two mixes them
    mixed = []
    for grp, al in zip(groups, aliased):
        if al:
            a, b = grp[leaf_id[grp] == leaf_id[grp[0]]], grp[leaf_id[grp] != leaf_id[grp[0]]]
            k = min(a.size, b.size)
            grp = np.concatenate([np.stack([a[:k], b[:k]], 1).ravel(), a[k:], b[k:]])
        mixed.append(grp)
    return xyz, mixed, aliased


def outside_points(g, n, rng):
    """n points without a key: far away, and ON the grid's own faces (-0.5 and GridSize - 0.5 outer voxels from the origin:
    both round outward)"""
    o = origin_of(g)
    inside = o + rng.integers(0, (g - 1) * 32, (n, 3)) * STEP
    far = inside + np.array([1000.0, -500.0, 250.0])
    lower, upper = inside.copy(), inside.copy()
    lower[np.arange(n), np.arange(n) % 3] = o - RES / 2
    upper[np.arange(n), (np.arange(n) + 1) % 3] = o + RES * g - RES / 2
    pick = np.arange(n) % 3
    return np.where((pick == 0)[:, None], far, np.where((pick == 1)[:, None], lower, upper))


def arrange(runs, order, rng):
    """the runs' points (a list of xyz arrays) in one of the three arrival orders"""
    if order == "interleaved":
        frac = np.concatenate([(np.arange(len(r)) + 0.5) / len(r) for r in runs])
        vid = np.concatenate([np.full(len(r), j) for j, r in enumerate(runs)])
        return np.concatenate(runs)[np.lexsort((vid, frac))]
    xyz = np.concatenate([runs[j] for j in rng.permutation(len(runs))])
    return xyz[::-1] if order == "reversed" else xyz


def run_lengths(total, max_voxels):
    """RUNS and the runs that fill the batch up to `total` points"""
    rest = total - sum(RUNS)
    if max_voxels is None:
        fill, cycle, i = [], (1, 2, 3, 5, 8, 13, 21, 34, 55, 89), 0
        while sum(fill) < rest:
            fill.append(min(cycle[i % len(cycle)], rest - sum(fill)))
            i += 1
    else:
        k = max_voxels - len(RUNS)
        fill = [rest // k + (i % 5 - 2) * 7 for i in range(k)]
        fill[-1] += rest - sum(fill)
    assert sum(fill) == rest and min(fill) > 0
    return list(RUNS) + fill


def run_structure(g, order, max_voxels=None):
    """layer 1: two batches of 3 * 4096 + 1 points with the same runs in the same kind of order.  The second one puts the runs
    of 255 and 513 and every fifth of the filling runs on voxels the first did not touch, so that with MinFramesPerVoxel 1 the
    clean map (count > 1) is the voxels both Adds hit: a voxel counted twice by one Add, or not at all, shows in its bytes"""
    rng = np.random.default_rng(1000 + g * 10 + ("contiguous", "interleaved", "reversed").index(order))
    xyz, groups, aliased = keyed_pool(g)
    lengths = run_lengths(BATCH - TAIL, None if max_voxels is None else max_voxels - 12)  # (up to 12 more voxels in the second batch)
    chosen = rng.choice(len(groups), len(lengths), replace=False)
    if aliased.any():
        # the runs of 2, 257 and 513 (places 1, 4, 5) on keys that two leaves share
        al = rng.permutation(np.flatnonzero(aliased & ~np.isin(np.arange(len(groups)), chosen)))[:3]
        chosen[[1, 4, 5]] = al
    # the run of 256 (place 3) on a key of one leaf, beginning with two different points at exactly the same distance
    if aliased[chosen[3]]:
        chosen[3] = np.flatnonzero(~aliased & ~np.isin(np.arange(len(groups)), chosen))[0]
    grp = groups[chosen[3]]
    d = norm3(xyz[grp].astype(f32) - leaf_centres(xyz[grp], g, RES, LEAF, (0, 0, 0)))
    a, b = next((i, j) for i in range(grp.size) for j in range(i + 1, grp.size) if d[i] == d[j])
    groups[chosen[3]] = np.r_[grp[[a, b]], np.delete(grp, [a, b])]
    moved = [2, 5] + list(range(len(RUNS), len(lengths), 5))[:10]
    unused = ~np.isin(np.arange(len(groups)), chosen)
    second = chosen.copy()
    second[moved] = rng.permutation(np.flatnonzero(unused & ~aliased))[: len(moved)]
    if aliased.any():
        second[5] = rng.permutation(np.flatnonzero(unused & aliased))[0]
    ops = []
    for rep in range(2):
        runs = []
        for place, (grp_id, n) in enumerate(zip(second if rep else chosen, lengths)):
            grp = groups[grp_id]
            start = 0 if place == 3 else int(rng.integers(0, grp.size)) & ~1
            runs.append(xyz[grp[(start + np.arange(n)) % grp.size]])
        runs.append(outside_points(g, TAIL, rng))
        ops.append(Add(make_points(arrange(runs, order, rng), rng, t0=rep * 1.0), time=0.1 * (rep + 1)))
    wants = ("straddle", "headless", "run4097", "tail", "tie_intensity", "tie_distance", "count_split", "alias" if g <= 8 else "no_alias")
    if order == "interleaved":
        wants += ("spread",)
    name = f"runs_{order}_g{g}" + ("" if max_voxels is None else f"_{max_voxels}voxels")
    return Case(name, 1, g, ops, wants, min_frames=1, centroid=max_voxels is not None and max_voxels <= 64)


def one_voxel(g, n):
    """layer 1: n points in one voxel, twice; the voxel is one that two leaves share, and from two points on the run mixes them.
    MinFramesPerVoxel 1: the clean map is empty after the first Add and the voxel after the second"""
    rng = np.random.default_rng(2000 + g * 1000 + n)
    xyz, groups, aliased = keyed_pool(g)
    grp = groups[int(np.flatnonzero(aliased)[7])]
    ops = []
    for rep in range(2):
        pts = xyz[grp[(rep + np.arange(n)) % grp.size]]
        ops.append(Add(make_points(pts[::-1] if rep else pts, rng, t0=rep * 1.0), time=0.1 * (rep + 1)))
    wants = ("one_voxel",) + (("tie_intensity", "alias") if n >= 255 else ())
    return Case(f"one_voxel_{n}_g{g}", 1, g, ops, wants, min_frames=1, centroid=True)


def some_groups(g, rng, n, want_aliased=3):
    xyz, groups, aliased = keyed_pool(g)
    chosen = rng.choice(len(groups), n, replace=False)
    if aliased.any():
        chosen[:want_aliased] = rng.permutation(np.flatnonzero(aliased & ~np.isin(np.arange(len(groups)), chosen)))[:want_aliased]
    return xyz, [groups[c] for c in chosen]


def intensity_patterns(g):
    """layer 2: runs whose intensities rise, fall, peak in the middle, and repeat their maximum (the first must win)"""
    rng = np.random.default_rng(3000 + g)
    patterns = [list(range(9)), list(range(8, -1, -1)), [1, 2, 7, 3, 0], [1, 5, 3, 5, 2, 5], [4, 4, 4], [0, 6, 6, 1, 6, 2, 6]]
    xyz, groups = some_groups(g, rng, 8 * len(patterns), 6)
    runs, inten = [], []
    for j, grp in enumerate(groups):
        pat = patterns[j % len(patterns)]
        runs.append(xyz[grp[np.arange(len(pat)) % grp.size]])
        inten.append(np.array(pat, f32))
    ops = []
    for rep, order in enumerate(("contiguous", "interleaved")):
        tagged = [np.c_[r, i] for r, i in zip(runs, inten)]
        a = arrange(tagged, order, rng)
        p = make_points(a[:, :3], rng, t0=rep * 1.0)
        p["intensity"] = a[:, 3].astype(f32)
        ops.append(Add(p, time=0.1 * (rep + 1)))
    return Case(f"intensity_patterns_g{g}", 2, g, ops, ("tie_intensity", "alias" if g <= 8 else "no_alias"), min_frames=1, centroid=True)


def mirrored_pairs(g):
    """layer 2: per voxel two points whose y and z offsets are swapped -- exactly the same distance to the point CENTER_POINT
    measures to: the first must win --, then one strictly closer, then the pair again the other way round"""
    rng = np.random.default_rng(4000 + g)
    o = origin_of(g)
    runs = []
    for j in range(60):
        out = rng.integers(0, g, 3)
        inn = rng.integers(-3, 4, 3)
        base = o + RES * out + LEAF * inn
        a, b = STEP * (1 - j % 2), -STEP  # (0.125 or 0, and -0.125): a != b, both well inside the leaf
        p1, p2 = base + [0.0, a, b], base + [0.0, b, a]
        closer = base + [-STEP, -STEP, -STEP]
        runs.append(np.array([p1, p2, closer, p2, p1][: 5 if j % 3 else 2]))
    ops = []
    for rep, order in enumerate(("contiguous", "interleaved")):
        ops.append(Add(make_points(arrange(runs, order, rng), rng, t0=rep * 1.0), time=0.1 * (rep + 1)))
    return Case(f"mirrored_pairs_g{g}", 2, g, ops, ("tie_distance",), min_frames=1, centroid=True)


def second_add(g):
    """layer 2: an Add of long runs, then long runs onto half of its voxels and some new ones, then onto a quarter and half of
    the new ones: the `exists` branch of the fold.  MinFramesPerVoxel 2: the counts 1, 2 and 3 decide the clean map and both
    passes of the sub-map extraction (min_nb reached by the first pass, and not)"""
    rng = np.random.default_rng(5000 + g)
    lengths = [1, 2, 300, 700, 257, 1100] + [3] * 120
    xyz, groups = some_groups(g, rng, len(lengths) + 40, 4)
    ops = []
    n, everything = len(lengths), (np.full(3, -1000, f32), np.full(3, 1000, f32))
    selections = [list(range(n)), list(range(0, n, 2)) + list(range(n, n + 40)), list(range(0, n, 4)) + list(range(n, n + 40, 2))]
    for rep, sel in enumerate(selections):
        runs = [xyz[groups[j][(rep + np.arange(lengths[j % n])) % groups[j].size]] for j in sel]
        runs.append(outside_points(g, 301, rng))
        ops.append(Add(make_points(arrange(runs, ("interleaved", "contiguous", "reversed")[rep], rng), rng, t0=rep * 1.0), time=0.1 * (rep + 1)))
        if rep:
            ops += [SubMap(*everything, min_nb) for min_nb in (0, 5, 10**6)]
    return Case(f"second_add_g{g}", 2, g, ops, ("straddle", "headless", "tie_intensity", "count_split", "submap_passes", "alias" if g <= 8 else "no_alias"),
                min_frames=2)


def fixed_voxels(g):
    """layer 2: an Add, a fixed Add onto half of its voxels and some new ones (runs of several points: the first arrival makes
    the voxel fixed, the rest of the run is refused), then two Adds onto the fixed voxels alone: nothing changes, not the time"""
    rng = np.random.default_rng(6000 + g)
    xyz, groups = some_groups(g, rng, 60, 4)
    lengths = [1, 2, 5, 300, 9, 3]

    def batch(sel, order, t0):
        runs = [xyz[groups[j][(j + np.arange(lengths[j % len(lengths)])) % groups[j].size]] for j in sel]
        return make_points(arrange(runs, order, rng), rng, t0=t0, levels=9)

    ops = [Add(batch(range(0, 40), "contiguous", 0.0), time=0.1),
           Add(batch(range(0, 60, 2), "interleaved", 1.0), fixed=True, time=0.2),
           Add(batch(range(0, 60, 2), "reversed", 2.0), time=0.3, still_valid=(0, 1, 2, 3)),
           Add(batch(range(0, 60, 4), "interleaved", 3.0), fixed=True, time=0.4, still_valid=(0, 1, 2, 3)),
           Add(batch(range(0, 60), "contiguous", 4.0), time=0.5)]
    return Case(f"fixed_voxels_g{g}", 2, g, ops, ("straddle", "count_split", "alias" if g <= 8 else "no_alias"), min_frames=1, centroid=True)


def no_change(g):
    """layer 2: an Add that changes no point -- FIRST onto existing voxels, MAX_INTENSITY with nothing but ties (every voxel
    holds intensity 3 after the first Add, the second brings 3 alone, to three voxels in four: MinFramesPerVoxel 1 keeps those)"""
    rng = np.random.default_rng(7000 + g)
    xyz, groups = some_groups(g, rng, 70, 4)
    lengths = [4, 6, 260, 5, 600]
    ops = []
    for rep in range(2):
        runs, inten = [], []
        for j, grp in enumerate(groups):
            if rep and j % 4 == 3:
                continue
            n = lengths[j % len(lengths)]
            runs.append(np.c_[xyz[grp[(rep + np.arange(n)) % grp.size]], np.full(n, 3.0) if rep else (np.arange(n) + j) % 4])
        a = arrange(runs, ("contiguous", "interleaved")[rep], rng)
        p = make_points(a[:, :3], rng, t0=rep * 1.0)
        p["intensity"] = a[:, 3].astype(f32)
        ops.append(Add(p, time=0.1 * (rep + 1), still_valid=(0, 2) if rep else ()))
    return Case(f"no_change_g{g}", 2, g, ops, ("straddle", "headless", "tie_intensity", "count_split"), min_frames=1)


def face_coordinates(g):
    """coordinates of one axis ON faces: of leaves (leaf quotient +-0.5, +-1.5, +-3.5), of outer voxels (quotient k +- 0.5,
    below and above the grid position 0), and of the grid itself (-0.5 and GridSize - 0.5)"""
    o = origin_of(g)
    leaf = [o + RES * k + s * (LEAF / 2 + LEAF * j) for k in (0, 1, g - 1) for s in (-1, 1) for j in (0, 1, 3)]
    outer = [o + RES * k - RES / 2 for k in range(1, g)]
    grid = [o - RES / 2, o + RES * g - RES / 2]
    return leaf, outer, grid


def faces(g):
    """layer 3: every face coordinate on one axis with plain coordinates on the others, and corners with faces on all three;
    every point three times (different intensities), added in two orders"""
    rng = np.random.default_rng(8000 + g)
    o = origin_of(g)
    leaf, outer, grid = face_coordinates(g)
    F = np.array(sorted(set(leaf + outer + grid)))
    plain = np.array([[o + RES * k + a, o + RES * k2 + b] for k, a, k2, b in ((0, -0.625, g - 1, 0.875), (g // 2, 0.875, 0, -0.625), (g - 1, 0.375, 1, -1.125))])
    pts = []
    for d in range(3):
        for pl in plain:
            p = np.zeros((F.size, 3))
            p[:, d] = F
            p[:, (d + 1) % 3], p[:, (d + 2) % 3] = pl
            pts.append(p)
    small = np.array([leaf[0], leaf[3], leaf[-1], outer[0], outer[-1], grid[0], grid[1], o + RES * (g // 2) - LEAF / 2])
    cx, cy, cz = np.meshgrid(small, small, small, indexing="ij")
    pts.append(np.stack([cx.ravel(), cy.ravel(), cz.ravel()], 1))
    pts = np.repeat(np.concatenate(pts), 3, axis=0)
    ops = [Add(make_points(pts[rng.permutation(len(pts))], rng, t0=0.0), time=0.1), Add(make_points(pts[::-1], rng, t0=1.0), time=0.2)]
    return Case(f"faces_g{g}", 3, g, ops, ("faces", "tie_intensity"))


ROLL_STEPS = [  # (offset / resolution per axis, the box is larger than the grid, through Add(roll=True))
    ((0.5, -0.5, 1.5), False, True), ((-1.5, 1.5, -0.5), False, False), ((-0.5, 0.5, -1.5), False, True),
    ((1.5, -1.5, 0.5), False, False), ((0.5, -0.5, 0.0), True, False), ((-1.5, 1.5, 0.5), True, True),
    ((-0.5, -1.5, 1.5), True, False), ((1.5, 0.5, -0.5), True, True)]


def rolls(g):
    """layer 3: Add(roll=True) and Roll with boxes whose clamped offset over the resolution is exactly +-0.5 and +-1.5 on each
    axis: a box smaller than the grid sticking out on one side (one clamp), and a box larger than the grid (both clamps: the
    mean of the two overhangs decides)"""
    rng = np.random.default_rng(9000 + g)
    xyz, groups = some_groups(g, rng, 1200, 0)
    base = np.concatenate([xyz[grp[:2]] for grp in groups])
    ops = [Add(make_points(base[rng.permutation(len(base))], rng), time=0.05)]
    pos, h = np.zeros(3), g / 2 * RES
    for step, (q, larger, through_add) in enumerate(ROLL_STEPS):
        q = np.array(q)
        if larger:
            mn, mx = pos - h - (10.0 - RES * q), pos + h + (10.0 + RES * q)
        else:
            mx = np.where(q > 0, pos + h + RES * q, np.where(q < 0, pos - h + RES * q + 3.0, pos + 1.5))
            mn = mx - 3.0
        got, vox, _ = roll_offset(mn, mx, g, RES, pos)
        assert np.array_equal(got, q.astype(f32)), (got, q)
        if through_add:
            inner = mn + rng.integers(0, ((mx - mn) / STEP).astype(int) + 1, (600, 3)) * STEP
            cloud = np.concatenate([[mn], inner, [mx]])
            ops.append(Add(make_points(np.repeat(cloud, 2, axis=0), rng, t0=step * 1.0), time=0.1 * (step + 1), roll=True))
        else:
            ops.append(Roll(mn.astype(f32), mx.astype(f32)))
        pos = pos + vox * RES
    return Case(f"rolls_g{g}", 3, g, ops, ("roll_halves", "roll_clamps"))


def submaps(g):
    """layer 3: MinFramesPerVoxel 3, one cloud added three times and another once; boxes with corners ON outer faces, beyond the
    grid on either side and in the wrong order, with min_nb unfiltered (-1), reached by the first pass, and not reached"""
    rng = np.random.default_rng(10000 + g)
    xyz, groups = some_groups(g, rng, 900, 0)
    a = np.concatenate([xyz[grp[:1]] for grp in groups[:500]])
    b = np.concatenate([xyz[grp[:1]] for grp in groups[400:]])
    ops = [Add(make_points(a[rng.permutation(len(a))], rng, t0=rep * 1.0), time=0.1 * (rep + 1)) for rep in range(3)]
    ops.append(Add(make_points(b, rng, t0=3.0), time=0.4))
    o = origin_of(g)
    face = lambda k: o + RES * k - RES / 2  # noqa: E731  (the face between outer voxels k - 1 and k)
    v = lambda *c: np.array(c, f32)  # noqa: E731
    boxes = [(v(face(0), face(0), face(0)), v(face(g), face(g), face(g))),        # the grid's own faces: all of it
             (v(face(1), face(0), face(2)), v(face(g - 1), face(g), face(g - 2))),  # ON outer faces inside
             (v(face(g // 2), face(1), face(1)), v(face(g // 2), face(g - 1), face(g - 1))),  # lo == hi ON a face
             (v(-1000, -1000, -1000), v(1000, 1000, 1000)),                      # beyond the grid on both sides
             (v(-1000, -1000, -1000), v(-500, -500, -500)), (v(500, 500, 500), v(1000, 1000, 1000)),  # all of it beyond one side
             (v(-1000, face(1), o), v(o, 1000, face(g - 1))),
             (v(face(g - 1), face(g - 1), face(g - 1)), v(face(1), face(1), face(1))),  # lo > hi: empty and invalid
             (v(face(1), face(g - 1), face(1)), v(face(g - 1), face(1), face(g - 1)))]  # ... on one axis only
    for mn, mx in boxes:
        for min_nb in (-1, 0, 5, 10**6):
            ops.append(SubMap(mn, mx, min_nb))
    return Case(f"submaps_g{g}", 3, g, ops, ("submap_faces", "submap_passes", "submap_wrong_order"), min_frames=3)


# ---- layer 4: several maps in one launch ------------------------------------------------------------------------------------
STAGED = ((1, 4097, 300), (4097, 1, 0), (0, 0, 257))  # points per map (= keypoint type) in each of the three launches


@dataclass
class MultiCase:
    """three maps of one context with different parameters: what each holds before (one nothing, one more than 1024 voxels:
    two chunks of old voxels), and `rounds`: per launch the points of every map and the time -- the three launches of STAGED,
    twice.  `maps[i]` is the same history for map i alone, as a Case of Add(roll=True) calls."""
    name: str
    maps: list    # Case per map (its first ops: the calls before the launches)
    before: list  # how many of maps[i].ops come before the launches
    rounds: list  # (time, [points of map 0, 1, 2])


def several_maps():
    rng = np.random.default_rng(11000)
    spec = [(6, 2, 0), (7, 3, 3), (12, 1, 0)]  # GridSize, Sampling, MinFramesPerVoxel
    pools = [some_groups(g, rng, 1800 if i == 1 else 400, 4) for i, (g, _, _) in enumerate(spec)]
    ops = [[], [], []]
    # map 0 starts empty; map 1 with 1500 voxels; map 2 with 300
    for i, n in ((1, 1500), (2, 300)):
        xyz, groups = pools[i]
        ops[i].append(Add(make_points(np.concatenate([xyz[grp[:1]] for grp in groups[:n]]), rng), time=0.01, roll=False))
    before = [len(o) for o in ops]
    rounds = []
    for rep in range(2):
        for r, counts in enumerate(STAGED):
            t = 0.1 * (1 + rep * len(STAGED) + r)
            batch = []
            for i, n in enumerate(counts):
                xyz, groups = pools[i]
                # runs of up to a few dozen points; the second time round one outer voxel further along x
                vox = rng.choice(len(groups), max(1, n // 40), replace=False)
                idx = np.concatenate([groups[v][: 1 + (j % 11)] for j, v in enumerate(vox)] * 40)[:n] if n else np.zeros(0, int)
                pts = make_points(xyz[idx] + [RES * rep, 0.0, 0.0], rng, t0=t)
                assert pts.size == n
                batch.append(pts[rng.permutation(n)])
                if n:
                    ops[i].append(Add(batch[-1], time=t, roll=True))
            rounds.append((t, batch))
    maps = [Case(f"several_maps_map{i}", 4, g, ops[i], (), min_frames=mf, sampling=s) for i, (g, s, mf) in enumerate(spec)]
    return MultiCase("several_maps", maps, before, rounds)


def _build():
    cases = []
    for g in GRID_SIZES:
        for order in ("contiguous", "interleaved", "reversed"):
            cases.append(run_structure(g, order))
    for n in (1, 255, 256, 257):
        cases.append(one_voxel(6, n))
    for g in (6, 12):
        for order in ("contiguous", "interleaved", "reversed"):
            cases.append(run_structure(g, order, max_voxels=64))
    for g in GRID_SIZES:
        cases += [intensity_patterns(g), mirrored_pairs(g), second_add(g), fixed_voxels(g), no_change(g)]
    for g in GRID_SIZES:
        cases += [faces(g), rolls(g), submaps(g)]
    return cases


CASES = _build()
MULTI = several_maps()


# ---- what a case is there to contain ------------------------------------------------------------------------------------------
def sorted_batch(points, g, position=(0, 0, 0)):
    """keys of the batch in the order the sort leaves (by key, then arrival), the arrival index of every place, and the runs
    of equal valid keys as (start, end) places"""
    keys = voxel_keys(xyz_of(points), g, RES, LEAF, position)
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    valid = int((sk != NO_KEY).sum())
    starts = np.flatnonzero(np.r_[True, sk[1:valid] != sk[: valid - 1]]) if valid else np.zeros(0, int)
    ends = np.r_[starts[1:], valid] if valid else starts
    return sk, order, starts, ends, valid


def straddles(start, end, of):
    """a multiple m of `of` with start < m < end: places m - 1 and m both belong to [start, end)"""
    m = (start // of + 1) * of
    return m < end


def run_statistics(points, g, position=(0, 0, 0)):
    """the figures of the table in the suite's description: share of points that share a voxel with an earlier one, longest
    run, runs that straddle a 256-place border, borders among the places with a key"""
    sk, order, starts, ends, valid = sorted_batch(points, g, position)
    n_straddling = int(sum(straddles(s, e, BLOCK) for s, e in zip(starts, ends)))
    return dict(points=int(points.size), keyed=valid, voxels=int(starts.size), shared=float((valid - starts.size) / max(valid, 1)),
                longest=int((ends - starts).max()) if starts.size else 0, straddling=n_straddling, borders=int((valid - 1) // BLOCK))


def vacuity_problems(case):
    """what `case.wants` names and the case does not contain; an empty list is a sound case"""
    g = case.grid_size
    found = set()
    adds = []  # the Adds in front of the first move of the grid: the grid position is the origin
    for op in case.ops:
        if isinstance(op, Roll) or (isinstance(op, Add) and op.roll):
            break
        if isinstance(op, Add):
            adds.append(op.points)
    # the counts (one per Add and voxel, none for a voxel that holds a fixed point): at some call the clean map -- count >
    # MinFramesPerVoxel -- is a non-empty proper subset of the map, and both the kept and the dropped voxels include one whose
    # run in some Add so far was 255 points or longer or straddled a border of 256 places
    count, fixed_now, hard, passes = {}, {}, set(), set()
    for op in case.ops:
        if isinstance(op, Roll) or (isinstance(op, Add) and op.roll):
            break
        if isinstance(op, SubMap):
            # corners ON outer faces; a first pass that reaches min_nb and one that does not, while the second pass has something
            # to add; a box in the wrong order
            origin = grid_origin(g, RES, (0, 0, 0))
            idx = np.array(sorted(count), np.uint64) >> np.uint64(32)
            cnt = np.array([count[k] for k in sorted(count)])
            idx = idx.astype(np.int64)
            o3 = np.stack([idx % g, (idx // g) % g, idx // (g * g)], 1).reshape(-1, 3)
            lo = np.maximum(position_to_voxel(op.mn, origin, RES), 0)
            hi = np.minimum(position_to_voxel(op.mx, origin, RES), g - 1)
            q = np.r_[(op.mn - origin) / f32(RES), (op.mx - origin) / f32(RES)]
            if np.all(np.abs(q - np.trunc(q)) == 0.5):
                found.add("submap_faces")
            if np.any(op.mn > op.mx):
                found.add("submap_wrong_order")
            inside = np.all((o3 >= lo) & (o3 <= hi), axis=1)
            first, second = int((inside & (cnt >= case.min_frames)).sum()), int((inside & (cnt < case.min_frames)).sum())
            if op.min_nb > 0 and second > 0:
                passes.add("reached" if first >= op.min_nb else "short" if first > 0 else "none")
            if {"reached", "short"} <= passes:
                found.add("submap_passes")
            continue
        sk, _, starts, ends, _ = sorted_batch(op.points, g)
        for s, e in zip(starts, ends):
            k = int(sk[s])
            if e - s >= 255 or straddles(s, e, BLOCK):
                hard.add(k)
            if not fixed_now.get(k, False):
                count[k] = count.get(k, 0) + 1
                fixed_now[k] = op.fixed
        kept = {k for k, c in count.items() if c > case.min_frames}
        if 0 < len(kept) < len(count) and hard & kept and hard - kept:
            found.add("count_split")
    mixes = []
    for pts in adds:
        sk, order, starts, ends, valid = sorted_batch(pts, g)
        n = pts.size
        lengths = ends - starts
        xyz = xyz_of(pts)
        out, inn, inside, centre = voxel_coords(xyz, g, RES, LEAF, (0, 0, 0))
        if any(straddles(s, e, BLOCK) for s, e in zip(starts, ends)):
            found.add("straddle")
        # a block of 256 places with a key in every place and no head among them: it begins behind the run's head and ends
        # inside the run
        if any((s // BLOCK + 2) * BLOCK <= e for s, e in zip(starts, ends)):
            found.add("headless")
        if lengths.size and lengths.max() >= SORT_RUN + 1:
            found.add("run4097")
        if n - valid >= 300 and straddles(valid, n, BLOCK) and straddles(valid, n, SORT_RUN):
            found.add("tail")
        if starts.size == 1 and valid == n:
            found.add("one_voxel")
        # every run of 255 points or more has points in every full sort run, and the longest owns the place left over
        full = n // SORT_RUN
        long_runs = [(s, e) for s, e in zip(starts, ends) if e - s >= 255]
        if long_runs and full >= 3 and all(set(range(full)) <= set((order[s:e] // SORT_RUN).tolist()) for s, e in long_runs):
            last = np.flatnonzero(order == n - 1)[0]
            owner = [e - s for s, e in zip(starts, ends) if s <= last < e]
            if n % SORT_RUN == 0 or (owner and owner[0] >= SORT_RUN + 1):
                found.add("spread")
        # ties that decide: a point whose intensity equals the run's maximum so far / whose distance equals the distance of
        # the closest so far (another point, same leaf)
        inten = pts["intensity"]
        dist = norm3(xyz - leaf_centres(xyz, g, RES, LEAF, (0, 0, 0)))
        leaf_id = leaf_ids(inn)
        mix = False
        for s, e in zip(starts, ends):
            idx = order[s:e]
            if e - s < 2:
                continue
            v = inten[idx]
            if np.any(v[1:] == np.maximum.accumulate(v)[:-1]):
                found.add("tie_intensity")
            one_leaf = np.all(leaf_id[idx] == leaf_id[idx[0]])
            mix = mix or not one_leaf
            d = dist[idx]
            best = np.minimum.accumulate(d)[:-1]
            arg = np.array([int(np.argmin(d[: j + 1])) for j in range(len(d) - 1)]) if one_leaf and np.any(d[1:] == best) else None
            if arg is not None:
                tie = np.flatnonzero(d[1:] == best)
                if any(np.any(xyz[idx[t + 1]] != xyz[idx[arg[t]]]) for t in tie):
                    found.add("tie_distance")
        mixes.append(mix)
        # faces, per axis: leaf quotient -(m + 0.5) and +(m + 0.5); outer quotient k + 0.5 below and above the grid position;
        # the grid's own two faces
        origin = grid_origin(g, RES, (0, 0, 0))
        qo = (xyz - origin) / f32(RES)
        ql = (xyz - centre) / f32(LEAF)
        half = lambda q: np.abs(q - np.trunc(q)) == 0.5  # noqa: E731
        kinds = [inside[:, None] & half(ql) & (ql < 0), inside[:, None] & half(ql) & (ql > 0),
                 inside[:, None] & half(qo) & (xyz < 0), inside[:, None] & half(qo) & (xyz > 0),
                 qo == f32(-0.5), qo == f32(g - 0.5)]
        if all(k[:, d].any() for k in kinds for d in range(3)) and not inside[np.any(kinds[4] | kinds[5], axis=1)].any():
            found.add("faces")
    if adds and any(mixes):
        found.add("alias")
    if adds and not any(mixes):
        found.add("no_alias")
    # the moves: offset over resolution on every axis takes each of +-0.5 and +-1.5; some box overhangs the grid on both sides
    pos, seen_q, both = np.zeros(3, f32), [set(), set(), set()], False
    for op in case.ops:
        box = box_of(op.points) if isinstance(op, Add) and op.roll else (op.mn, op.mx) if isinstance(op, Roll) else None
        if box is None:
            continue
        q, vox, (down, up) = roll_offset(box[0], box[1], g, RES, pos)
        for d in range(3):
            seen_q[d].add(float(q[d]))
        both = both or bool(np.all((down < 0) & (up > 0)))
        pos = pos + vox.astype(f32) * f32(RES)
    if all({0.5, -0.5, 1.5, -1.5} <= s for s in seen_q):
        found.add("roll_halves")
    if both:
        found.add("roll_clamps")
    return [w for w in case.wants if w not in found]


def multi_problems(multi):
    """the launches are the stated ones; before them one map is empty and one holds more than 1024 voxels"""
    problems = []
    counts = tuple(tuple(int(p.size) for p in batch) for _, batch in multi.rounds)
    if counts != STAGED + STAGED:
        problems.append(f"staged counts {counts}")
    sizes = []
    for case, nb in zip(multi.maps, multi.before):
        s = Statement(case.grid_size, 0)
        for op in case.ops[:nb]:
            s.add(op.points, fixed=op.fixed, time=op.time, roll=op.roll)
        sizes.append(s.size())
    if min(sizes) != 0 or max(sizes) <= 1024 or len(set(sizes)) != 3:
        problems.append(f"map sizes before the launches {sizes}")
    if len({(c.grid_size, c.sampling, c.min_frames) for c in multi.maps}) != 3:
        problems.append("the maps share their parameters")
    return problems
