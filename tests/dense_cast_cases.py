"""Cases for rays cast through the dense map (lidarslam_amd/_dense_map.py: DenseMapHost.cast / .compare, dense_ray_steps with
`extend`; lidarslam_amd/csrc/lsa_dense_cast.hip: k_dense_cast, k_dense_compare).  Needs neither a GPU nor the native library.

Builds on tests/dense_carve_cases.py: a ray case's origin and point are a cast's origin and target, and its carve keywords
become cast keywords -- margin_leaves = m is extend = -m * LEAF (len + extend is len - margin to the bit), so that K.walk(name)
is the cast's walk too and the cases that cast no ray for their margin are the "tt not > 0" cases of a negative extend."""
import numpy as np

import dense_carve_cases as K
from dense_map_cases import LEAF
from lidarslam_amd._dense_map import DenseMapHost, dense_index_keys, dense_ray_steps

F32 = np.float32
EXTENDS = (0.0, LEAF, float("inf"), -2.0 * LEAF)


def xyz(points):
    """(n, 3) float32 of LidarPoints"""
    return np.stack([points["x"], points["y"], points["z"]], axis=1).astype(F32)


def cast_case(name):
    """(origin (1, 3), target (1, 3), cast keywords) of the ray case `name` under its own margin"""
    o, p, kw = K.RAY_CASES[name]
    return np.array([o], F32), np.array([p], F32), dict(extend=-kw.get("margin_leaves", 2.0) * LEAF, max_range=kw.get("max_range", 30.0))


def cast_walks(origins, targets, leaf=LEAF, extend=0.0, max_range=30.0):
    """per ray the list of (voxel, t_in, t_out) the cast's walk visits on an empty map, None for no ray"""
    tg = np.asarray(targets, F32).reshape(-1, 3)
    out = [None] * len(tg)
    for rays, index, t_in, t_out in dense_ray_steps(K.cloud(tg), origins, leaf, max_range=max_range, extend=extend):
        for r, i, a, b in zip(rays.tolist(), index.tolist(), t_in.tolist(), t_out.tolist()):
            if out[r] is None:
                out[r] = []
            out[r].append((tuple(i), a, b))
    return out


def key_of(index):
    return int(dense_index_keys(np.asarray([index], np.int64))[0])


def host_with(indices, frame=0, leaf=LEAF):
    """a host map holding one point in each of these voxels"""
    h = DenseMapHost(leaf)
    if len(indices):
        h.insert(K.voxel_points(np.asarray(indices, np.int64).reshape(-1, 3), leaf=leaf), frame)
    return h


def thinned_scene(name):
    """ray_scene(name) thinned to every third voxel: hits fall at varied depths, and some rays miss"""
    return K.ray_scene(name)[::3]


def state(h, min_frames=1, ratio=-1.0):
    """everything of a host map no cast may change"""
    pts, vox = h.get(min_frames, ratio)
    return pts.tobytes(), vox.tobytes(), h.sources(min_frames, ratio).tobytes(), h.misses(min_frames, ratio).tobytes(), h.rays, h.last_frame, h.skipped, h.pruned


# ---- the independent statement: slabs, no walk ---------------------------------------------------------------------------------
def slab_first_hits(origins, targets, voxels, leaf, near=1e-9):
    """For segments o -> t (extend 0, within the range) and occupied voxel indices (m, 3): per ray (index of the voxel of
    smallest entry parameter or -1, left_out) from (lo - o) / d and (hi - o) / d per voxel and axis.  A ray is left out when
    two entries lie within `near`, a voxel is grazed within `near`, or a voxel begins or ends within `near` of the segment's ends."""
    o = np.asarray(origins, F32).astype(np.float64)[:, None, :]
    t = np.asarray(targets, F32).astype(np.float64)[:, None, :]
    lo = np.asarray(voxels, np.float64)[None, :, :] * leaf
    d = t - o
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = (lo - o) / d, (lo + leaf - o) / d
    enter, leave = np.minimum(a, b).max(axis=2), np.maximum(a, b).min(axis=2)
    met = (enter <= leave) & (leave >= 0.0) & (enter <= 1.0)
    entry = np.where(met, np.maximum(enter, 0.0), np.inf)
    first = np.where(met.any(axis=1), entry.argmin(axis=1), -1)
    ordered = np.sort(entry, axis=1)
    with np.errstate(invalid="ignore"):
        close = (ordered[:, 1] - ordered[:, 0] < near) & np.isfinite(ordered[:, 1])
    doubtful = (np.abs(leave - enter) < near) | (np.abs(enter - 1.0) < near) | (np.abs(leave) < near)
    return first, close | doubtful.any(axis=1)


# ---- the scene of the carve cases, for compare ------------------------------------------------------------------------------
def wall_only():
    """(host map holding the wall alone, the wall's points)"""
    _, wall, _ = K.scene()
    pts = K.voxel_points(wall)
    h = DenseMapHost(LEAF)
    h.insert(pts, 0)
    return h, pts


# one point each: in the empty space in front of the wall, behind the wall by more than a leaf, beyond the range
IN_FRONT, BEHIND, BEYOND = (3.25, 0.25, 0.25), (8.25, 0.25, 0.25), (40.25, 0.25, 0.25)


def box_points(n=40, ahead=6.0, side=1.0, seed=8):
    """n LidarPoints of a box of `side` metres `ahead` of the sensor, in the sensor's frame, within the frame's time span"""
    rng = np.random.default_rng(seed)
    p = K.cloud(rng.uniform(-side / 2, side / 2, (n, 3)) + np.array([ahead, 0.0, 0.0]), intensity=np.full(n, 90.0))
    p["time"] = -0.05
    p["laser_id"] = np.arange(n) % 16
    p["label"] = 0
    return p
