"""The dense point-cloud map: registered frames voxel-hashed on the device (lsa_dense_map_*, lsa_slam_*dense_map*).

DenseMapHost is the numpy statement of what the map computes; the device table (lidarslam_amd/csrc/lsa_dense_*.hip) is
held to it byte for byte, on points, voxel records, sources and misses (free-space carving: DenseMapHost.carve) and on the
normals computed from the table (DenseMapHost.normals, dense_normals) and on the floor plan rasterised from it
(DenseMapHost.grid, dense_grid: elevation, ground, and a 2-D occupancy grid of occupied / free / unknown cells).  DenseMap is
the table alone on a Context; dense_map(slam, ...) and its neighbours reach the pipeline's map (Slam.set_param("DenseMap", 1
or 2)).
"""
import ctypes as C
import os

import numpy as np

from ._abi import LsaError, _error, lib
from ._native import LIB_PATH, POINT_DTYPE, pose16, ptr
from ._pcd import PCD_BINARY

# lsa_dense_voxel_t (include/lidarslam_amd.h)
dense_voxel_dtype = np.dtype([("key", "<u8"), ("count", "<u4"), ("frames", "<u4"), ("first_frame", "<i4"), ("last_frame", "<i4")])

# lsa_dense_normal_t (include/lidarslam_amd.h)
dense_normal_dtype = np.dtype([("normal_x", "<f4"), ("normal_y", "<f4"), ("normal_z", "<f4"), ("curvature", "<f4"), ("neighbors", "<u4")])

# lsa_dense_cell_t and lsa_dense_grid_info_t (include/lidarslam_amd.h)
dense_cell_dtype = np.dtype([("elevation", "<f4"), ("ground", "<f4"), ("top", "<f4"), ("floor_voxels", "<u4"), ("obstacle_voxels", "<u4")])
dense_grid_info_dtype = np.dtype([("cx0", "<i4"), ("cy0", "<i4"), ("width", "<i4"), ("height", "<i4"), ("resolution", "<f8"), ("origin_x", "<f8"), ("origin_y", "<f8")])

# lsa_dense_hit_t (include/lidarslam_amd.h): what a ray cast through the map reports
dense_hit_dtype = np.dtype([("key", "<u8"), ("entry", "<f4"), ("exit", "<f4"), ("depth", "<f4"), ("steps", "<i4"), ("source", "<i4"), ("status", "<i4")])

DENSE_INDEX_RANGE = 1 << 20  # voxel indices lie in [-2^20, 2^20)
DENSE_NO_NORMAL = 0x7FC00000  # the four floats of a voxel without a normal: this quiet NaN
DENSE_GRID_ABSENT = 0x7FC00000  # a cell's elevation, ground or top that is not there: the same quiet NaN
DENSE_GRID_MAX_CELLS = 1 << 24  # "GridMaxCells" of a map that was not told otherwise
GRID_OCCUPIED, GRID_FREE, GRID_UNKNOWN = 100, 0, -1  # nav_msgs/OccupancyGrid
PGM_OCCUPIED, PGM_FREE, PGM_UNKNOWN = 0, 254, 205  # map_server's grey levels


class DenseGridParams(C.Structure):
    """lsa_dense_grid_params_t"""

    _fields_ = [
        ("min_height", C.c_double), ("max_height", C.c_double), ("max_miss_ratio", C.c_double), ("window", C.c_double * 4),
        ("cell_leaves", C.c_int32), ("ground_radius", C.c_int32), ("min_obstacle_voxels", C.c_int32), ("min_frames", C.c_int32), ("use_window", C.c_int32),
    ]


class DenseCastParams(C.Structure):
    """lsa_dense_cast_params_t"""

    _fields_ = [
        ("max_range", C.c_double), ("extend", C.c_double), ("max_miss_ratio", C.c_double),
        ("min_frames", C.c_int32), ("use_before", C.c_int32), ("before", C.c_int32), ("reserved", C.c_int32),
    ]


class DenseGridInfo(C.Structure):
    """lsa_dense_grid_info_t"""

    _fields_ = [("cx0", C.c_int32), ("cy0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("resolution", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double)]


def dense_intensity_code(intensity):
    """The order in which intensities are compared, as unsigned codes (f2ou of lsa_wave.h): a larger float has a larger code,
    -0.0 ranks below +0.0, and a NaN is coded 0, below -inf."""
    v = np.ascontiguousarray(intensity, np.float32)
    u = v.view(np.uint32)
    code = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(v), np.uint32(0), code)


def dense_voxel_keys(points, leaf):
    """(keys, taking_part) of LidarPoints: i_a = floor((double)p_a / (double)leaf); a point whose coordinate is not finite or
    whose index lies outside [-2^20, 2^20) takes no part.  key = ((iz + 2^20) << 42) | ((iy + 2^20) << 21) | (ix + 2^20)."""
    pts = np.ascontiguousarray(points, POINT_DTYPE)
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64)
    ok = np.isfinite(xyz).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        idx = np.floor(xyz / np.float64(leaf))
    ok &= ((idx >= -DENSE_INDEX_RANGE) & (idx < DENSE_INDEX_RANGE)).all(axis=1)
    i = np.where(ok[:, None], idx, 0.0).astype(np.int64) + DENSE_INDEX_RANGE
    keys = (i[:, 2].astype(np.uint64) << np.uint64(42)) | (i[:, 1].astype(np.uint64) << np.uint64(21)) | i[:, 0].astype(np.uint64)
    return keys, ok


def dense_ray_steps(points, origins, leaf, margin_leaves=2.0, max_range=30.0, stride=1, extend=None, info=None):
    """The walk of DenseMapHost.carve, for all rays at once.  Yields (ray, index): `ray` the indices into `points` of the rays
    that visit a voxel in this round, `index` (len(ray), 3) int64 the voxel each visits.  The first round is every ray's
    start voxel; a ray of k steps appears in the first k + 1 rounds.  A point that casts no ray never appears.

    With `extend` (metres, may be +inf or negative) the walk is DenseMapHost.cast's: reach = len + extend in place of len -
    margin_leaves * leaf, and every round yields (ray, index, t_in, t_out): the step parameter in [0, 1] at which the ray
    entered the voxel (the tmax of the step that entered it, before tdelta was added; 0 for the start voxel) and at which it
    leaves it (the smallest tmax among the axes with steps left, 1 when none is left).  `info`, a dict, is given "ray",
    "len" and "tt" of the rays that are cast before the first round."""
    pts = np.ascontiguousarray(points, POINT_DTYPE)
    n = pts.size
    org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    if org.shape[0] != n and org.shape[0] != 1:
        raise ValueError("one origin, or one per point")
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride >= 1")
    sel = np.arange(0, n, stride)
    if sel.size == 0:
        return
    leaf = np.float64(leaf)
    p = np.stack([pts["x"], pts["y"], pts["z"]], axis=1)[sel].astype(np.float64)
    o = (org[sel] if org.shape[0] == n else np.repeat(org, sel.size, axis=0)).astype(np.float64)
    with np.errstate(all="ignore"):
        d = p - o
        length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        reach = length - np.float64(margin_leaves) * leaf if extend is None else length + np.float64(extend)
        t = np.where(reach < np.float64(max_range), reach, np.float64(max_range))
        ok = np.isfinite(o).all(axis=1) & np.isfinite(p).all(axis=1) & (t > 0) & (length > 0)  # (len 0 and a margin: t <= 0 already)
        e = o + d * (t / length)[:, None]
        f0, f1 = np.floor(o / leaf), np.floor(e / leaf)
        ok &= ((f0 >= -DENSE_INDEX_RANGE) & (f0 < DENSE_INDEX_RANGE) & (f1 >= -DENSE_INDEX_RANGE) & (f1 < DENSE_INDEX_RANGE)).all(axis=1)
        at = np.flatnonzero(ok)
        if at.size == 0:
            return
        ray, o, e = sel[at], o[at], e[at]
        i, i1 = f0[at].astype(np.int64), f1[at].astype(np.int64)
        left = np.abs(i1 - i)
        step = np.sign(i1 - i)
        tmax = ((i + (step > 0)).astype(np.float64) * leaf - o) / (e - o)
        tdelta = leaf / np.abs(e - o)
    if info is not None:
        info.update(ray=ray.copy(), len=length[at].copy(), tt=t[at].copy())
    t_in = np.zeros(ray.size)
    while True:
        # among the axes with steps left the smallest tmax, the earlier axis on a tie; -1: no step is left
        a = np.full(ray.size, -1)
        best = np.zeros(ray.size)
        for ax in range(3):
            take = (left[:, ax] > 0) & ((a < 0) | (tmax[:, ax] < best))
            a = np.where(take, ax, a)
            best = np.where(take, tmax[:, ax], best)
        if extend is None:
            yield ray, i.copy()
        else:
            yield ray, i.copy(), t_in.copy(), np.where(a >= 0, best, 1.0)
        go = a >= 0
        if not go.any():
            return
        if not go.all():
            ray, i, left, step, tmax, tdelta, a, best = ray[go], i[go], left[go], step[go], tmax[go], tdelta[go], a[go], best[go]
        rows = np.arange(ray.size)
        i[rows, a] += step[rows, a]
        with np.errstate(all="ignore"):
            tmax[rows, a] += tdelta[rows, a]
        left[rows, a] -= 1
        t_in = best


def _dense_cast_check(leaf, max_range, extend, min_frames, compare=False):
    """ValueError for what DenseMapHost.cast / .compare refuse (the device: LSA_E_ARG)"""
    if not (np.isfinite(max_range) and max_range > 0 and np.float64(max_range) / np.float64(leaf) <= 4096.0):
        raise ValueError("max_range finite, positive and at most 4096 leaves")
    if np.isnan(extend) or (compare and not (np.isfinite(extend) and extend >= 0)):
        raise ValueError("the tolerance finite and >= 0" if compare else "extend is NaN")
    if int(min_frames) < 1:
        raise ValueError("min_frames >= 1")


def _scan_targets_numpy(pose, elevations, n_azimuth):
    T = np.asarray(pose, np.float64).reshape(4, 4)
    el = np.asarray(elevations, np.float64).reshape(-1)
    az = 6.283185307179586476925286766559 * np.arange(int(n_azimuth), dtype=np.float64) / np.float64(int(n_azimuth)) if int(n_azimuth) > 0 else np.zeros(0)
    v = np.stack([np.cos(el)[:, None] * np.cos(az)[None, :], np.cos(el)[:, None] * np.sin(az)[None, :], np.sin(el)[:, None] * np.ones_like(az)[None, :]], axis=-1).reshape(-1, 3)
    out = np.stack([((T[k, 0] * v[:, 0] + T[k, 1] * v[:, 1]) + T[k, 2] * v[:, 2]) + T[k, 3] for k in range(3)], axis=1)
    return T[:3, 3].astype(np.float32).reshape(1, 3), out.astype(np.float32)


def scan_targets(pose, elevations, n_azimuth):
    """(origin (1, 3) float32, targets (n_rings * n_azimuth, 3) float32, ring-major) of a spinning sensor at `pose` (4x4): the
    origin is the pose's translation narrowed to float, target (r, c) the pose applied to (cos el_r cos az_c, cos el_r sin az_c,
    sin el_r), az_c = 2 pi c / n_azimuth, in double, narrowed to float.  The floats are lsa_scan_targets' (host only), the one
    place where a sensor model becomes rays; without the built library, the same statement in numpy (whose cos and sin may
    differ from the C library's in the last bit)."""
    el = np.ascontiguousarray(elevations, np.float64).reshape(-1)
    n_azimuth = int(n_azimuth)
    if n_azimuth < 0:
        raise ValueError("n_azimuth >= 0")
    if not os.path.exists(LIB_PATH):
        return _scan_targets_numpy(pose, el, n_azimuth)
    T = pose16(pose)
    origin, targets = np.zeros((1, 3), np.float32), np.zeros((max(el.size * n_azimuth, 1), 3), np.float32)
    rc = lib().lsa_scan_targets(ptr(T), ptr(el) if el.size else ptr(np.zeros(1)), el.size, n_azimuth, ptr(origin), ptr(targets))
    if rc != 0:
        raise _error("lsa_scan_targets", rc, "bad argument")
    return origin, targets[: el.size * n_azimuth].copy()


def dense_index_keys(index):
    """the keys of voxel indices (n, 3) int64 in [-2^20, 2^20)"""
    i = np.asarray(index, np.int64) + DENSE_INDEX_RANGE
    return (i[:, 2].astype(np.uint64) << np.uint64(42)) | (i[:, 1].astype(np.uint64) << np.uint64(21)) | i[:, 0].astype(np.uint64)


def eigh_eig(cov):
    """The eigen step by numpy.linalg.eigh, in the layout of lsa_selftest_numerics fn 3: (m, 6) Sym3 doubles xx xy xz yy yz zz
    -> (m, 12) l0 l1 l2 e0 e1 e2.  NOT the byte definition of dense_normals (that is eigen33<double> of lsa_device_math.h):
    normals agree with it up to sign and the bound of tests/test_dense_normals_host.py."""
    c = np.ascontiguousarray(cov, np.float64).reshape(-1, 6)
    A = c[:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3)
    out = np.zeros((c.shape[0], 12))
    if c.shape[0]:
        w, v = np.linalg.eigh(A)
        out[:, :3] = w
        out[:, 3:] = np.transpose(v, (0, 2, 1)).reshape(-1, 9)
    return out


def dense_normal_sums(points, keys, radius_leaves=2):
    """(k (n,) int64, s (n, 3), S (n, 6)) of dense_normals: per voxel the neighbour count and the sums of d and of its
    products xx xy xz yy yz zz over the neighbours, in cell order"""
    pts = np.ascontiguousarray(points, POINT_DTYPE)
    K = np.ascontiguousarray(keys, np.uint64)
    n = K.size
    r = int(radius_leaves)
    p = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64)
    mask = np.uint64((1 << 21) - 1)
    idx = np.stack([(K & mask), ((K >> np.uint64(21)) & mask), (K >> np.uint64(42)) & mask], axis=1).astype(np.int64) - DENSE_INDEX_RANGE
    k = np.zeros(n, np.int64)
    s, S = np.zeros((n, 3)), np.zeros((n, 6))
    if n == 0:
        return k, s, S
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                cell = idx + np.array([dx, dy, dz], np.int64)
                inside = ((cell >= -DENSE_INDEX_RANGE) & (cell < DENSE_INDEX_RANGE)).all(axis=1)
                want = dense_index_keys(np.where(inside[:, None], cell, 0))
                at = np.minimum(np.searchsorted(K, want), n - 1)
                found = inside & (K[at] == want)
                # (a sum that began at +0.0 is never -0.0, so the +0.0 a cell without a neighbour adds changes no bit)
                d = np.where(found[:, None], p[at] - p, 0.0)
                k += found
                s += d
                for c, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                    S[:, c] += d[:, a] * d[:, b]
    return k, s, S


def dense_normal_covariances(k, s, S):
    """(m, 6) Sym3 xx xy xz yy yz zz of dense_normals from the sums of dense_normal_sums (k > 0): C_ab = S_ab / k - (s_a / k) * (s_b / k)"""
    kk = np.asarray(k).astype(np.float64)
    m = np.asarray(s, np.float64) / kk[:, None]
    cov = np.empty((kk.size, 6))
    for c, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        cov[:, c] = np.asarray(S, np.float64)[:, c] / kk - m[:, a] * m[:, b]
    return cov


def dense_normals(points, keys, sources, radius_leaves=2, min_neighbors=5, viewpoints=None, first_frame=0, eig=None):
    """The definition of the dense map's normals over an export: points, keys (ascending) and sources of the voxels that count.
    One dense_normal_dtype record per voxel, in their order; see DenseMapHost.normals."""
    r = int(radius_leaves)
    if r not in (1, 2):
        raise ValueError("radius_leaves is 1 or 2")
    min_neighbors = int(min_neighbors)
    if min_neighbors < 3 or min_neighbors > (2 * r + 1) ** 3:
        raise ValueError("min_neighbors between 3 and (2 * radius_leaves + 1)^3")
    vp = None
    if viewpoints is not None:
        vp = np.asarray(viewpoints)
        if vp.ndim != 2 or vp.shape[1] != 3:
            raise ValueError("viewpoints of shape (n, 3)")
        vp = np.ascontiguousarray(vp, np.float32)
    pts = np.ascontiguousarray(points, POINT_DTYPE)
    n = pts.size
    out = np.zeros(n, dense_normal_dtype)
    if n == 0:
        return out
    k, s, S = dense_normal_sums(pts, keys, r)
    floats = np.full((n, 4), DENSE_NO_NORMAL, np.uint32)
    out["neighbors"] = k
    fit = np.flatnonzero(k >= min_neighbors)
    if fit.size:
        cov = dense_normal_covariances(k[fit], s[fit], S[fit])
        E = np.asarray((eigh_eig if eig is None else eig)(cov), np.float64).reshape(-1, 12)
        lam, e0 = E[:, :3], E[:, 3:6].copy()
        ok = np.isfinite(E[:, :6]).all(axis=1)
        if vp is not None and vp.shape[0] > 0:
            c = np.clip(np.asarray(sources, np.int64)[fit] - int(first_frame), 0, vp.shape[0] - 1)
            p = np.stack([pts["x"], pts["y"], pts["z"]], axis=1).astype(np.float64)[fit]
            w = vp[c].astype(np.float64) - p
            with np.errstate(invalid="ignore", over="ignore"):
                dot = (e0[:, 0] * w[:, 0] + e0[:, 1] * w[:, 1]) + e0[:, 2] * w[:, 2]
                e0 = np.where((dot < 0)[:, None], -e0, e0)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = (lam[:, 0] + lam[:, 1]) + lam[:, 2]
            curv = np.where(t > 0, np.abs(lam[:, 0] / np.where(t > 0, t, 1.0)).astype(np.float32), np.float32(0))
            res = np.concatenate([e0.astype(np.float32), curv.astype(np.float32)[:, None]], axis=1)
        good = fit[ok]
        floats[good] = np.ascontiguousarray(res[ok]).view(np.uint32)
    for c, name in enumerate(("normal_x", "normal_y", "normal_z", "curvature")):
        out[name] = floats[:, c].view(np.float32)
    return out


def dense_order_decode(code):
    """the floats of ordered codes (ou2f of lsa_wave.h), the inverse of dense_intensity_code on numbers"""
    u = np.ascontiguousarray(code, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def dense_grid_check(cell_leaves=2, ground_radius=2, min_height=0.2, max_height=2.0, min_obstacle_voxels=1, window=None):
    """ValueError for what DenseMapHost.grid refuses (the device: LSA_E_ARG)"""
    if not 1 <= int(cell_leaves) <= 64:
        raise ValueError("cell_leaves between 1 and 64")
    if not 0 <= int(ground_radius) <= 16:
        raise ValueError("ground_radius between 0 and 16 cells")
    if not (np.isfinite(min_height) and np.isfinite(max_height) and 0 <= min_height < max_height):
        raise ValueError("0 <= min_height < max_height, both finite")
    if int(min_obstacle_voxels) < 1:
        raise ValueError("min_obstacle_voxels >= 1")
    if window is not None:
        w = np.asarray(window, np.float64).reshape(-1)
        if w.size != 4 or not np.isfinite(w).all() or w[0] > w[2] or w[1] > w[3]:
            raise ValueError("window = (x_min, y_min, x_max, y_max), finite, x_min <= x_max, y_min <= y_max")


def dense_grid_window_cells(leaf, cell_leaves, window):
    """(cx0, cy0, cx1, cy1) of a window in metres, None for one without a cell: per end i = floor((double)v / (double)leaf),
    the two IEEE operations of the keys; a window wholly below or above the index range has no cell, any other is clamped
    to it; c = i // cell_leaves"""
    w = np.asarray(window, np.float64).reshape(4)
    cl = int(cell_leaves)
    ends = []
    for lo, hi in ((w[0], w[2]), (w[1], w[3])):
        with np.errstate(over="ignore"):
            i0, i1 = np.floor(lo / np.float64(leaf)), np.floor(hi / np.float64(leaf))
        if i1 < -DENSE_INDEX_RANGE or i0 >= DENSE_INDEX_RANGE:
            return None
        i0, i1 = (int(min(max(i, -DENSE_INDEX_RANGE), DENSE_INDEX_RANGE - 1)) for i in (i0, i1))
        ends.append((i0 // cl, i1 // cl))
    return ends[0][0], ends[1][0], ends[0][1], ends[1][1]


def dense_grid(points, keys, leaf, cell_leaves=2, ground_radius=2, min_height=0.2, max_height=2.0, min_obstacle_voxels=1, window=None, max_cells=DENSE_GRID_MAX_CELLS):
    """The definition of the dense map's floor plan over an export: points and keys of the voxels that count, in any order.
    -> (info: a dense_grid_info_dtype scalar, cells: (height, width) dense_cell_dtype, state: (height, width) int8); see
    DenseMapHost.grid.  OverflowError when width * height > max_cells."""
    dense_grid_check(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, window)
    cl, r = int(cell_leaves), int(ground_radius)
    pts = np.ascontiguousarray(points, POINT_DTYPE)
    K = np.ascontiguousarray(keys, np.uint64)
    mask = np.uint64((1 << 21) - 1)
    cx = ((K & mask).astype(np.int64) - DENSE_INDEX_RANGE) // cl  # floor division: voxel -1 is in cell -1
    cy = (((K >> np.uint64(21)) & mask).astype(np.int64) - DENSE_INDEX_RANGE) // cl
    z = pts["z"].astype(np.float32)
    code = dense_intensity_code(z)
    info = np.zeros((), dense_grid_info_dtype)
    info["resolution"] = np.float64(cl) * np.float64(leaf)
    if window is not None:
        extent = dense_grid_window_cells(leaf, cl, window)
    else:
        extent = (int(cx.min()), int(cy.min()), int(cx.max()), int(cy.max())) if K.size else None
    if extent is None:
        return info, np.zeros((0, 0), dense_cell_dtype), np.zeros((0, 0), np.int8)
    cx0, cy0, cx1, cy1 = extent
    W, H = cx1 - cx0 + 1, cy1 - cy0 + 1
    if W * H > int(max_cells):
        raise OverflowError(f"a grid of {W} x {H} cells is over max_cells = {int(max_cells)}")
    info["cx0"], info["cy0"], info["width"], info["height"] = cx0, cy0, W, H
    info["origin_x"] = np.float64(cx0 * cl) * np.float64(leaf)
    info["origin_y"] = np.float64(cy0 * cl) * np.float64(leaf)
    none = np.uint32(0xFFFFFFFF)
    # column pass, over the window expanded by the radius: the smallest code of a column
    col = np.full((H + 2 * r, W + 2 * r), none, np.uint32)
    ex, ey = cx - (cx0 - r), cy - (cy0 - r)
    near = (ex >= 0) & (ex < W + 2 * r) & (ey >= 0) & (ey < H + 2 * r)
    np.minimum.at(col, (ey[near], ex[near]), code[near])
    # ground pass: the smallest code of the (2r + 1)^2 columns around; min is exact and associative, so rows first
    rows = col[:, 0:W].copy()
    for d in range(1, 2 * r + 1):
        np.minimum(rows, col[:, d:d + W], out=rows)
    ground = rows[0:H].copy()
    for d in range(1, 2 * r + 1):
        np.minimum(ground, rows[d:d + H], out=ground)
    # band pass: every voxel of the window against the ground of its cell (which has one: its own column at least)
    inside = np.flatnonzero((cx >= cx0) & (cx <= cx1) & (cy >= cy0) & (cy <= cy1))
    at = (cy[inside] - cy0, cx[inside] - cx0)
    h = z[inside].astype(np.float64) - dense_order_decode(ground[at]).astype(np.float64)
    low = h <= np.float64(min_height)
    mid = ~low & (h <= np.float64(max_height))
    floor_voxels, obstacle_voxels, top = np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32), np.zeros((H, W), np.uint32)
    np.add.at(floor_voxels, (at[0][low], at[1][low]), np.uint32(1))
    np.add.at(obstacle_voxels, (at[0][mid], at[1][mid]), np.uint32(1))
    np.maximum.at(top, (at[0][mid], at[1][mid]), code[inside][mid])
    cells = np.zeros((H, W), dense_cell_dtype)
    elevation = col[r:r + H, r:r + W]
    absent = np.uint32(DENSE_GRID_ABSENT)
    cells["elevation"] = np.where(elevation != none, dense_order_decode(elevation).view(np.uint32), absent).view(np.float32)
    cells["ground"] = np.where(ground != none, dense_order_decode(ground).view(np.uint32), absent).view(np.float32)
    cells["top"] = np.where(top != 0, dense_order_decode(top).view(np.uint32), absent).view(np.float32)
    cells["floor_voxels"], cells["obstacle_voxels"] = floor_voxels, obstacle_voxels
    state = np.where(obstacle_voxels >= np.uint32(int(min_obstacle_voxels)), GRID_OCCUPIED, np.where(floor_voxels >= 1, GRID_FREE, GRID_UNKNOWN)).astype(np.int8)
    return info, cells, state


def occupancy_pgm(state):
    """(height, width) uint8 as <prefix>.pgm holds it: occupied 0, free 254, unknown 205, image row 0 the grid's last row"""
    s = np.asarray(state, np.int8)
    return np.where(s == GRID_OCCUPIED, PGM_OCCUPIED, np.where(s == GRID_FREE, PGM_FREE, PGM_UNKNOWN)).astype(np.uint8)[::-1]


def write_occupancy_pgm(prefix, info, state):
    """<prefix>.pgm and <prefix>.yaml of a grid, written from Python: the statement of what lsa_occupancy_write writes, byte
    for byte.  Nothing is written for a grid without cells; returns the number of cells"""
    s = np.asarray(state, np.int8)
    h, w = (int(info["height"]), int(info["width"]))
    if h * w == 0:
        return 0
    prefix = os.fspath(prefix)
    with open(prefix + ".pgm", "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h))
        f.write(occupancy_pgm(s.reshape(h, w)).tobytes())
    with open(prefix + ".yaml", "w") as f:
        f.write("image: %s.pgm\nresolution: %s\norigin: [%s, %s, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n" % (
            os.path.basename(prefix), "%.17g" % float(info["resolution"]), "%.17g" % float(info["origin_x"]), "%.17g" % float(info["origin_y"])))
    return h * w


def read_occupancy_pgm(prefix):
    """(state (height, width) int8 with row 0 the grid's first row again, resolution, (origin_x, origin_y)) of <prefix>.pgm and
    <prefix>.yaml; ValueError for a file that is not a map of save_grid's"""
    prefix = os.fspath(prefix)
    data = open(prefix + ".pgm", "rb").read()
    head = data.split(b"\n", 3)
    if len(head) < 4 or head[0] != b"P5" or head[2] != b"255":
        raise ValueError(prefix + ".pgm: not a binary PGM of maxval 255")
    w, h = (int(v) for v in head[1].split())
    grey = np.frombuffer(head[3], np.uint8)
    if grey.size != w * h:
        raise ValueError(prefix + ".pgm: %d bytes of pixels for %d x %d" % (grey.size, w, h))
    grey = grey.reshape(h, w)[::-1]
    known = (grey == PGM_OCCUPIED) | (grey == PGM_FREE) | (grey == PGM_UNKNOWN)
    if not known.all():
        raise ValueError(prefix + ".pgm: a grey level that is none of 0, 254, 205")
    state = np.where(grey == PGM_OCCUPIED, GRID_OCCUPIED, np.where(grey == PGM_FREE, GRID_FREE, GRID_UNKNOWN)).astype(np.int8)
    fields = {}
    for line in open(prefix + ".yaml"):
        name, _, value = line.partition(":")
        fields[name.strip()] = value.strip()
    if fields.get("image") != os.path.basename(prefix) + ".pgm" or fields.get("negate") != "0":
        raise ValueError(prefix + ".yaml: not the description of " + prefix + ".pgm")
    origin = [float(v) for v in fields["origin"].strip("[]").split(",")]
    return state, float(fields["resolution"]), (origin[0], origin[1])


class DenseMapHost:
    """The definition.  State: key -> (point, count, frames, first_frame, last_frame, intensity code, source).

    insert(points, frame): world points as lsa_transform_frame writes them and an ordinal that must not decrease.  Within one
    call a voxel's winner is the point of largest intensity (dense_intensity_code: a NaN loses to every number), ties to
    the smallest index of the call; n_f is the number of the call's points in the voxel.  A new voxel takes the winner's 32
    bytes as they are, count = n_f, frames = 1, first_frame = last_frame = frame.  An existing one: count += n_f, frames += 1
    unless last_frame == frame, last_frame = frame, and the point is replaced only when the winner's intensity is strictly
    greater -- the earlier frame keeps ties.  Nothing depends on the order in which the points of one call arrive.
    source is the ordinal of the call whose point the voxel holds: set when the voxel is made or its point replaced.

    reproject(corrections, first_frame): the map under a corrected trajectory.  This moves what the map kept -- one point per
    voxel, moved by the correction of the frame that measured it; it is not a rebuild from raw frames: two neighbouring
    surface voxels may merge, and the voxel between them may stay empty until it is seen again.

    carve(points, origins, frame, ...): free space.  Beside the above a voxel has misses (u32, 0 when made) and miss_frame
    (none when made).  Every point with index % stride == 0 casts a ray from its origin o to the point p, both float widened
    to double, everything in double and without contraction: d = p - o, len = sqrt((dx*dx + dy*dy) + dz*dz), t = min(len -
    margin_leaves * leaf, max_range).  No ray when a coordinate is not finite, t is not > 0, or a start or end index lies
    outside [-2^20, 2^20).  e = o + d * (t / len); i0 = floor(o / leaf), i1 = floor(e / leaf); per axis left = |i1 - i0|,
    step = sign(i1 - i0) and, where left > 0, tmax = ((i0 + (step > 0)) * leaf - o) / (e - o), tdelta = leaf / |e - o|.
    The ray visits i0 and then, exactly left_x + left_y + left_z times, steps along the axis of smallest tmax among those
    with left > 0 (ties to x, then y): i[a] += step[a], tmax[a] += tdelta[a], left[a] -= 1, and visits i.  It ends in i1.
    A visited voxel that exists, with last_frame != frame and miss_frame != frame, takes misses += 1 (modulo 2^32) and
    miss_frame = frame: one count an ordinal, whatever the number of rays and calls, and none in an ordinal that hit it.
    Nothing depends on the order of the rays.  carve makes, moves and removes no voxel and touches no point and no record.
    The ordinal must not be below the map's last one (nor be -2^31, which the device keeps for "none") and becomes the last.

    get / sources / misses (min_frames, max_miss_ratio): the voxels with frames >= min_frames and, for a ratio >= 0,
    (double)misses <= max_miss_ratio * (double)frames.  prune removes the others for good.

    normals(radius_leaves, min_neighbors, min_frames, max_miss_ratio, viewpoints, first_frame, eig): one record (normal,
    curvature, neighbors) per voxel of get(min_frames, max_miss_ratio), in its order, from the voxels' kept points.  For a
    voxel of index (ix, iy, iz) and point p the cells (ix+dx, iy+dy, iz+dz), dz, dy, dx in -r .. r with dx fastest (ascending
    key order), are visited; a cell with an index outside [-2^20, 2^20) is skipped, and a cell is a neighbour when its voxel
    exists and passes the same predicate -- the voxel itself is one.  With q the neighbour's point, all in double, from
    +0.0, without contraction and in that order: d = (double)q - (double)p, s_a += d_a, S_ab += d_a * d_b (ab = xx xy xz yy
    yz zz, the product rounded, then added), k the count = neighbors.  k < min_neighbors: the four floats are the quiet NaN
    0x7fc00000.  Otherwise m = s / k, C_ab = S_ab / k - m_a * m_b, eigen33<double>(C) of lsa_device_math.h gives l0 <= l1 <=
    l2 and e0; a non-finite eigenvalue or e0 gives that NaN too.  With viewpoints (n > 0, float32 (n, 3)): c = clamp(source
    - first_frame, 0, n - 1), w = (double)viewpoints[c] - p, dot = (e0x*wx + e0y*wy) + e0z*wz, and dot < 0 negates every
    component of e0 (anything else keeps eigen33's sign).  normal = (float)e0, t = (l0 + l1) + l2, curvature = t > 0 ?
    (float)|l0 / t| : 0 (PCL's surface variation).  Nothing depends on the order of the voxels; no state changes.
    `eig` is the eigen step, (m, 6) -> (m, 12) in the layout of lsa_selftest_numerics fn 3; None is numpy.linalg.eigh
    (eigh_eig), which is NOT the byte definition.

    grid(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, min_frames, max_miss_ratio, window): the floor
    plan, from the voxels of get(min_frames, max_miss_ratio) alone.  A voxel (ix, iy, iz) -- the indices of its key -- belongs
    to cell (ix // cell_leaves, iy // cell_leaves), floor division.  Codes are dense_intensity_code's (f2ou: -0.0 below +0.0).
    Column: a cell's elevation is the kept point z (the float of the slot) of smallest code among its voxels.  Ground:
    ground(c) is the smallest-code elevation over the (2 * ground_radius + 1)^2 cells around c that have a column, c among
    them, whether or not they lie inside the extent; none when none has one.  Band: per voxel h = (double)z -
    (double)ground(cell); h <= min_height is a floor voxel, min_height < h <= max_height an obstacle voxel, above that it is
    ignored; top is the obstacle z of largest code; the counts are uint32.  State (int8): 100 when obstacle_voxels >=
    min_obstacle_voxels, else 0 when floor_voxels >= 1, else -1 -- free means the floor was seen.  An absent float is the NaN
    0x7fc00000.  Extent: without a window the bounding box of the kept voxels' cells (no kept voxel: width = height = 0); with
    window = (x_min, y_min, x_max, y_max) the cells of dense_grid_window_cells, whatever the map holds, so that a window's
    answer is the crop of the whole grid's, to the byte.  resolution = cell_leaves * leaf, origin_x = (double)(cx0 *
    cell_leaves) * leaf; cells are row-major, row 0 is cy0, x fastest.  Nothing depends on the order of the voxels; no state
    changes.  ValueError for what dense_grid_check refuses, OverflowError above max_cells.

    cast(origins, targets, extend, max_range, min_frames, max_miss_ratio, before): what the map holds along a line.  Origin o
    and target t are float triples widened to double; everything in double, without contraction.  The geometry is carve's with
    len + extend in place of len - margin: d = t - o, len = sqrt((dx*dx + dy*dy) + dz*dz), reach = len + extend, tt = reach <
    max_range ? reach : max_range, e = o + d * (tt / len).  extend may be +inf (the ray runs to max_range, the target is only a
    direction) or negative.  No ray when a coordinate is not finite, tt is not > 0, len is 0, or a start or end index lies
    outside [-2^20, 2^20).  The walk is carve's, statement for statement (dense_ray_steps).  A visited voxel counts when it
    exists, frames >= min_frames, for max_miss_ratio >= 0 misses <= max_miss_ratio * frames (get's predicate) and, with `before`
    given, first_frame < before -- the map without what that ordinal and later ones created.  The first voxel that counts, in
    visiting order, is the hit and ends the walk.  One dense_hit_dtype record a ray: key (0 unless status 1); entry =
    (float)(t_in * tt), t_in the tmax of the step that entered the voxel before tdelta was added, 0 for the start voxel; exit =
    (float)(t_out * tt), t_out the smallest tmax among the axes with steps left when the voxel is visited, 1 when none is left;
    depth = (float)((((qx-ox)*dx + (qy-oy)*dy) + (qz-oz)*dz) / len) for the kept point q -- which may lie anywhere in its voxel,
    so depth need not lie between entry and exit; steps = voxels visited (up to and including the hit, the whole walk for a
    miss, 0 for no ray); source; status -1 no ray, 0 miss, 1 hit.  Everything but steps and status is 0 unless status is 1.
    Beside the records the hit voxels' LidarPoints, 32 zero bytes otherwise.

    compare(points, origins, tolerance, ...): one uint8 a point, from the ray of its origin to the point with extend =
    tolerance (finite, >= 0; default one leaf), decided in double before anything is narrowed: NOT_JUDGED 0 no ray, or len >
    max_range; UNMAPPED 2 no hit -- nothing that counts lies on the ray up to `tolerance` behind the point; THROUGH_MAP 3 a hit
    with t_out * tt < len - tolerance -- the ray left a voxel that counts more than the tolerance before it reached the point;
    CONSISTENT 1 every other hit.  And counts (4,) int64, the number of each.  Two limits of a test by voxels: at tolerance 0 a
    point exactly on a voxel face may end its walk one voxel short, because o + (t - o) need not be t in double; and at grazing
    incidence the ray meets occupied voxels of the same surface well before the point, so ground far away reads THROUGH_MAP at
    a small tolerance.  UNMAPPED is the robust label.
    Neither depends on the order of the rays, and neither changes any state -- no voxel, record, miss, `rays` or last_frame --
    but cast_rays, the rays the two have cast since the last clear."""

    NOT_JUDGED, CONSISTENT, UNMAPPED, THROUGH_MAP = 0, 1, 2, 3

    def __init__(self, leaf):
        if not (leaf > 0 and np.isfinite(leaf)):
            raise ValueError("leaf must be positive and finite")
        self.leaf = float(leaf)
        self.clear()

    def clear(self):
        self.voxels = {}
        self.skipped = 0
        self.dropped = 0
        self.rays = 0
        self.cast_rays = 0
        self.pruned = 0
        self.last_frame = None

    def size(self):
        return len(self.voxels)

    def insert(self, points, frame):
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        frame = int(frame)
        if self.last_frame is not None and frame < self.last_frame:
            raise ValueError("frame ordinals must not decrease")
        self.last_frame = frame
        keys, ok = dense_voxel_keys(pts, self.leaf)
        self.skipped += int((~ok).sum())
        taking = np.flatnonzero(ok)
        if taking.size == 0:
            return
        code = dense_intensity_code(pts["intensity"])[taking]
        k = keys[taking]
        # by key, then by falling intensity code, then by rising index: the first of every key is its winner
        order = np.lexsort((taking, np.iinfo(np.uint32).max - code, k))
        ks = k[order]
        first = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
        n_f = np.diff(np.concatenate([first, [ks.size]]))
        for key, at, n in zip(ks[first].tolist(), first.tolist(), n_f.tolist()):
            w = int(taking[order[at]])
            c = int(code[order[at]])
            v = self.voxels.get(key)
            if v is None:
                self.voxels[key] = [pts[w].copy(), n, 1, frame, frame, c, frame, 0, None]
                continue
            v[1] += n
            if v[4] != frame:
                v[2] += 1
                v[4] = frame
            if c > v[5]:
                v[0] = pts[w].copy()
                v[5] = c
                v[6] = frame

    def carve(self, points, origins, frame, margin_leaves=2.0, max_range=30.0, stride=1):
        """origins: (n, 3) or (1, 3) float32 world positions of the sensor per point; see the class"""
        frame = int(frame)
        if frame == -(1 << 31):
            raise ValueError("the ordinal -2^31 is not carved")
        if self.last_frame is not None and frame < self.last_frame:
            raise ValueError("frame ordinals must not decrease")
        rounds = list(dense_ray_steps(points, origins, self.leaf, margin_leaves, max_range, stride))
        self.last_frame = frame
        if not rounds:
            return
        self.rays += int(rounds[0][0].size)
        if not self.voxels:
            return
        have = np.fromiter(self.voxels.keys(), np.uint64, len(self.voxels))
        seen = np.unique(np.concatenate([np.unique(dense_index_keys(index)) for _, index in rounds]))
        for key in seen[np.isin(seen, have)].tolist():
            v = self.voxels[key]
            if v[4] != frame and v[8] != frame:
                v[7] = (v[7] + 1) & 0xFFFFFFFF
                v[8] = frame

    @staticmethod
    def _passes(v, min_frames, max_miss_ratio):
        return v[2] >= min_frames and (not max_miss_ratio >= 0 or float(v[7]) <= float(max_miss_ratio) * float(v[2]))

    def _kept(self, min_frames, max_miss_ratio):
        return sorted(k for k, v in self.voxels.items() if self._passes(v, min_frames, max_miss_ratio))

    def get(self, min_frames=1, max_miss_ratio=-1.0):
        """(points, voxels) of the voxels with frames >= min_frames and, for a ratio >= 0, misses <= ratio * frames, in
        ascending key order"""
        keys = self._kept(min_frames, max_miss_ratio)
        pts = np.zeros(len(keys), POINT_DTYPE)
        vox = np.zeros(len(keys), dense_voxel_dtype)
        for j, k in enumerate(keys):
            p, count, frames, first, last = self.voxels[k][:5]
            pts[j] = p
            vox[j] = (k, count, frames, first, last)
        return pts, vox

    def sources(self, min_frames=1, max_miss_ratio=-1.0):
        """the source of every voxel of get(min_frames, max_miss_ratio), in its order"""
        return np.array([self.voxels[k][6] for k in self._kept(min_frames, max_miss_ratio)], np.int32)

    def misses(self, min_frames=1, max_miss_ratio=-1.0):
        """the misses of every voxel of get(min_frames, max_miss_ratio), in its order"""
        return np.array([self.voxels[k][7] for k in self._kept(min_frames, max_miss_ratio)], np.uint32)

    def normals(self, radius_leaves=2, min_neighbors=5, min_frames=1, max_miss_ratio=-1.0, viewpoints=None, first_frame=0, eig=None):
        """dense_normal_dtype records of the voxels of get(min_frames, max_miss_ratio), in its order; see the class"""
        if int(min_frames) < 1:
            raise ValueError("min_frames >= 1")
        pts, vox = self.get(min_frames, max_miss_ratio)
        return dense_normals(pts, vox["key"], self.sources(min_frames, max_miss_ratio), radius_leaves, min_neighbors, viewpoints, first_frame, eig)

    def grid(self, cell_leaves=2, ground_radius=2, min_height=0.2, max_height=2.0, min_obstacle_voxels=1, min_frames=1, max_miss_ratio=-1.0, window=None,
             max_cells=DENSE_GRID_MAX_CELLS):
        """(info, cells (height, width) dense_cell_dtype, state (height, width) int8) of the voxels of get(min_frames,
        max_miss_ratio); see the class"""
        dense_grid_check(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, window)
        pts, vox = self.get(min_frames, max_miss_ratio)
        return dense_grid(pts, vox["key"], self.leaf, cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, window, max_cells)

    def _walk_to_hits(self, targets, origins, extend, max_range, min_frames, max_miss_ratio, before):
        """the walks of cast and compare: per ray status, steps, t_in, t_out, key of the hit, len and tt"""
        tg = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
        org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        n = tg.shape[0]
        if org.shape[0] != n and org.shape[0] != 1:
            raise ValueError("one origin, or one per ray")
        pts = np.zeros(n, POINT_DTYPE)
        pts["x"], pts["y"], pts["z"] = tg[:, 0], tg[:, 1], tg[:, 2]
        w = {"status": np.full(n, -1, np.int32), "steps": np.zeros(n, np.int32), "t_in": np.zeros(n), "t_out": np.zeros(n), "key": np.zeros(n, np.uint64),
             "len": np.zeros(n), "tt": np.zeros(n)}
        counting = np.array(sorted(k for k, v in self.voxels.items() if self._passes(v, min_frames, max_miss_ratio) and (before is None or v[3] < int(before))), np.uint64)
        info = {}
        done = np.zeros(n, bool)
        for turn, (ray, index, t_in, t_out) in enumerate(dense_ray_steps(pts, org, self.leaf, max_range=max_range, extend=extend, info=info)):
            if turn == 0:
                cast = info["ray"]  # the rays that are cast at all
                w["status"][cast], w["len"][cast], w["tt"][cast] = 0, info["len"], info["tt"]
                self.cast_rays += int(cast.size)
            live = ~done[ray]
            ray, index, t_in, t_out = ray[live], index[live], t_in[live], t_out[live]
            if ray.size == 0:
                break  # every ray that was cast has hit
            w["steps"][ray] += 1
            if counting.size:
                keys = dense_index_keys(index)
                at = np.minimum(np.searchsorted(counting, keys), counting.size - 1)
                hit = counting[at] == keys
                r = ray[hit]
                w["status"][r], w["t_in"][r], w["t_out"][r], w["key"][r] = 1, t_in[hit], t_out[hit], keys[hit]
                done[r] = True
        return w, org.astype(np.float64), tg.astype(np.float64)

    def cast(self, origins, targets, extend=0.0, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before=None):
        """(hits (n,) dense_hit_dtype, points (n,) LidarPoints) of the rays from origins ((n, 3) or (1, 3) float32) towards targets
        ((n, 3) float32); see the class"""
        _dense_cast_check(self.leaf, max_range, extend, min_frames)
        w, o, t = self._walk_to_hits(targets, origins, extend, max_range, min_frames, max_miss_ratio, before)
        n = t.shape[0]
        hits, points = np.zeros(n, dense_hit_dtype), np.zeros(n, POINT_DTYPE)
        hits["status"], hits["steps"] = w["status"], w["steps"]
        for r in np.flatnonzero(w["status"] == 1).tolist():
            v = self.voxels[int(w["key"][r])]
            ro = o[r if o.shape[0] == n else 0]
            d = t[r] - ro
            q = np.array([v[0]["x"], v[0]["y"], v[0]["z"]], np.float64)
            points[r] = v[0]
            hits["key"][r] = w["key"][r]
            hits["entry"][r] = np.float32(w["t_in"][r] * w["tt"][r])
            hits["exit"][r] = np.float32(w["t_out"][r] * w["tt"][r])
            hits["depth"][r] = np.float32((((q[0] - ro[0]) * d[0] + (q[1] - ro[1]) * d[1]) + (q[2] - ro[2]) * d[2]) / w["len"][r])
            hits["source"][r] = v[6]
        return hits, points

    def compare(self, points, origins, tolerance=None, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before=None):
        """(labels (n,) uint8, counts (4,) int64) of LidarPoints against the map, every point from its origin ((n, 3) or (1, 3)
        float32); tolerance in metres, None: one leaf; see the class"""
        tolerance = self.leaf if tolerance is None else float(tolerance)
        _dense_cast_check(self.leaf, max_range, tolerance, min_frames, compare=True)
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        targets = np.stack([pts["x"], pts["y"], pts["z"]], axis=1) if pts.size else np.zeros((0, 3), np.float32)
        w, _, _ = self._walk_to_hits(targets, origins, tolerance, max_range, min_frames, max_miss_ratio, before)
        through = w["t_out"] * w["tt"] < w["len"] - np.float64(tolerance)
        labels = np.where(w["status"] == 0, self.UNMAPPED, np.where(through, self.THROUGH_MAP, self.CONSISTENT))
        labels = np.where((w["status"] < 0) | (w["len"] > np.float64(max_range)), self.NOT_JUDGED, labels).astype(np.uint8)
        return labels, np.bincount(labels, minlength=4).astype(np.int64)

    def prune(self, min_frames=1, max_miss_ratio=-1.0):
        """removes every voxel get(min_frames, max_miss_ratio) leaves out; returns their number (also added to self.pruned)"""
        gone = [k for k, v in self.voxels.items() if not self._passes(v, min_frames, max_miss_ratio)]
        for k in gone:
            del self.voxels[k]
        self.pruned += len(gone)
        return len(gone)

    def reproject(self, corrections, first_frame=0):
        """corrections: (n, 16) float64, row-major 4x4 rigid transforms, entry j for ordinal first_frame + j.  Returns the
        number of voxels dropped (also added to self.dropped; skipped is not touched).

        Every voxel takes entry c = clamp(source - first_frame, 0, n - 1) and its point moves as rigid_apply of
        lsa_device_math.h moves it, in double, without contraction, narrowed to float: x' = (float)(((R0*x + R1*y) + R2*z)
        + t0), likewise y' and z' (so a -0.0 comes out +0.0 under the identity); the other 20 bytes are kept.  The new key
        is dense_voxel_keys of the moved point; a moved point that is not finite or lies outside the index range drops its
        voxel.  Voxels that arrive at one key merge: count is the sum modulo 2^32, first_frame the min, last_frame the
        max, frames = min(sum of frames, last_frame - first_frame + 1), point and source from the voxel of largest
        intensity code, ties to the smaller source, then to the smaller old key; misses is the sum modulo 2^32 and
        miss_frame the max.  Nothing depends on the order in which the voxels are visited; last_frame of the map, the guard on the ordinals, is unchanged."""
        D = np.ascontiguousarray(corrections, np.float64).reshape(-1, 16)
        n = D.shape[0]
        if n < 1:
            raise ValueError("at least one correction")
        old = sorted(self.voxels)
        if not old:
            return 0
        recs = [self.voxels[k] for k in old]
        pts = np.array([v[0] for v in recs], POINT_DTYPE)
        source = np.array([v[6] for v in recs], np.int64)
        T = D[np.clip(source - int(first_frame), 0, n - 1)]
        x, y, z = (pts[a].astype(np.float64) for a in ("x", "y", "z"))
        with np.errstate(over="ignore", invalid="ignore"):
            for row, a in enumerate(("x", "y", "z")):
                pts[a] = (((T[:, 4 * row] * x + T[:, 4 * row + 1] * y) + T[:, 4 * row + 2] * z) + T[:, 4 * row + 3]).astype(np.float32)
        keys, ok = dense_voxel_keys(pts, self.leaf)
        merged = {}
        for j in np.flatnonzero(ok).tolist():
            p, count, frames, first, last, code, src, misses, miss_frame = recs[j]
            rank = (-code, src, old[j])  # the smallest wins: largest code, then smaller source, then smaller old key
            m = merged.get(int(keys[j]))
            if m is None:
                merged[int(keys[j])] = [pts[j].copy(), count, frames, first, last, code, src, rank, misses, miss_frame]
                continue
            m[1] = (m[1] + count) & 0xFFFFFFFF
            m[2] += frames
            m[3], m[4] = min(m[3], first), max(m[4], last)
            m[8] = (m[8] + misses) & 0xFFFFFFFF
            if miss_frame is not None and (m[9] is None or miss_frame > m[9]):
                m[9] = miss_frame
            if rank < m[7]:
                m[0], m[5], m[6], m[7] = pts[j].copy(), code, src, rank
        self.voxels = {k: [m[0], m[1], min(m[2], m[4] - m[3] + 1), m[3], m[4], m[5], m[6], m[8], m[9]] for k, m in merged.items()}
        dropped = int((~ok).sum())
        self.dropped += dropped
        return dropped


class DenseMap:
    """The device table alone (lsa_dense_map_*) in the memory of `ctx`, a Context."""

    def __init__(self, ctx, leaf, **params):
        self.L = lib()
        self.ctx = ctx
        h = C.c_void_p()
        rc = self.L.lsa_dense_map_create(ctx.h, float(leaf), C.byref(h))
        if rc != 0:
            raise _error("lsa_dense_map_create", rc, self.L.lsa_last_error(ctx.h).decode())
        self.h = h
        for k, v in params.items():
            self.set(k, v)

    def close(self):
        if getattr(self, "h", None):
            if self.ctx.h:  # a map must go before its context; one that outlived it is dropped
                self.L.lsa_dense_map_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise _error(what, rc, self.L.lsa_last_error(self.ctx.h).decode())
        return rc

    def set(self, name, value):
        self._check(self.L.lsa_dense_map_set(self.h, name.encode(), float(value)), f"lsa_dense_map_set({name})")

    def get_param(self, name):
        return float(self.L.lsa_dense_map_get_param(self.h, name.encode()))

    def insert_points(self, points, frame):
        """world points of the caller's; raises LsaError with .code E_CAPACITY, the map untouched, when the table may not grow"""
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        self._check(self.L.lsa_dense_map_insert_points(self.h, ptr(pts) if pts.size else None, pts.size, int(frame)), "lsa_dense_map_insert_points")

    def insert_frame(self, frame, H0, H1=None, t0=0.0, t1=0.0, time_offset=0.0):
        """the context's current frame moved as lsa_transform_frame_at moves it, fused with the insertion"""
        interp = H1 is not None
        self._check(
            self.L.lsa_dense_map_insert_frame(self.h, int(interp), ptr(pose16(H0)), ptr(pose16(H1)) if interp else None, float(t0), float(t1), float(time_offset), int(frame)),
            "lsa_dense_map_insert_frame",
        )

    def size(self):
        return self._check(self.L.lsa_dense_map_size(self.h), "lsa_dense_map_size")

    def skipped(self):
        return self._check(self.L.lsa_dense_map_skipped(self.h), "lsa_dense_map_skipped")

    def bytes(self):
        return int(self.L.lsa_dense_map_bytes(self.h))

    def get(self, min_frames=1, max_miss_ratio=-1.0):
        """(points, voxels) with frames >= min_frames and, for a ratio >= 0, misses <= ratio * frames, in ascending key order"""
        cap = max(self.size(), 1)
        pts, vox = np.zeros(cap, POINT_DTYPE), np.zeros(cap, dense_voxel_dtype)
        n = self._check(self.L.lsa_dense_map_get_filtered(self.h, int(min_frames), float(max_miss_ratio), ptr(pts), ptr(vox), cap), "lsa_dense_map_get_filtered")
        return pts[:n].copy(), vox[:n].copy()

    def sources(self, min_frames=1, max_miss_ratio=-1.0):
        """int32 ordinals of the calls whose points the voxels of get(min_frames, max_miss_ratio) hold, in its order"""
        cap = max(self.size(), 1)
        out = np.zeros(cap, np.int32)
        n = self._check(self.L.lsa_dense_map_get_sources_filtered(self.h, int(min_frames), float(max_miss_ratio), ptr(out), cap), "lsa_dense_map_get_sources_filtered")
        return out[:n].copy()

    def misses(self, min_frames=1, max_miss_ratio=-1.0):
        """uint32 per voxel of get(min_frames, max_miss_ratio), in its order: the ordinals whose rays passed through it"""
        cap = max(self.size(), 1)
        out = np.zeros(cap, np.uint32)
        n = self._check(self.L.lsa_dense_map_get_misses(self.h, int(min_frames), float(max_miss_ratio), ptr(out), cap), "lsa_dense_map_get_misses")
        return out[:n].copy()

    def carve_points(self, points, origins, frame):
        """DenseMapHost.carve under the map's "CarveMarginLeaves", "CarveRange" and "CarveStride": world points of the caller's and
        the sensor's world position per point ((n, 3) float32) or for all of them ((1, 3))"""
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        self._check(
            self.L.lsa_dense_map_carve_points(self.h, ptr(pts) if pts.size else None, pts.size, ptr(org) if org.size else None, org.shape[0], int(frame)),
            "lsa_dense_map_carve_points",
        )

    def carve_frame(self, frame, H0, H1=None, t0=0.0, t1=0.0, time_offset=0.0):
        """the rays of the context's current frame moved as insert_frame moves it, every one from where the sensor stood at the
        point's time (frame_origins_at), fused with the walk"""
        interp = H1 is not None
        self._check(
            self.L.lsa_dense_map_carve_frame(self.h, int(interp), ptr(pose16(H0)), ptr(pose16(H1)) if interp else None, float(t0), float(t1), float(time_offset), int(frame)),
            "lsa_dense_map_carve_frame",
        )

    def prune(self, min_frames=1, max_miss_ratio=-1.0):
        """removes the voxels get(min_frames, max_miss_ratio) leaves out and shrinks the table to what is left; returns their
        number.  LsaError with .code E_CAPACITY, the map untouched, when the second table cannot be allocated"""
        removed = C.c_longlong(0)
        self._check(self.L.lsa_dense_map_prune(self.h, int(min_frames), float(max_miss_ratio), C.byref(removed)), "lsa_dense_map_prune")
        return int(removed.value)

    def reproject(self, corrections, first_frame=0):
        """the map under per-frame rigid corrections ((n, 16) or (n, 4, 4); entry j for ordinal first_frame + j), as
        DenseMapHost.reproject states it; returns the number of voxels dropped.  LsaError with .code E_CAPACITY, the map
        untouched, when the second table cannot be allocated; E_ARG for no corrections"""
        D = np.ascontiguousarray(corrections, np.float64).reshape(-1, 16)
        dropped = C.c_longlong(0)
        self._check(self.L.lsa_dense_map_reproject(self.h, ptr(D) if D.size else None, int(first_frame), D.shape[0], C.byref(dropped)), "lsa_dense_map_reproject")
        return int(dropped.value)

    def clear(self):
        self._check(self.L.lsa_dense_map_clear(self.h), "lsa_dense_map_clear")

    def normals(self, radius_leaves=2, min_neighbors=5, min_frames=1, max_miss_ratio=-1.0, viewpoints=None, first_frame=0):
        """dense_normal_dtype records of the voxels of get(min_frames, max_miss_ratio), in its order, as DenseMapHost.normals states
        them (with eigen33<double> as the eigen step); viewpoints: (n, 3) float32, entry j for ordinal first_frame + j.  LsaError
        with .code E_ARG, the map untouched, for what the statement refuses"""
        vp, n = _viewpoints(viewpoints)
        cap = max(self.size(), 1)
        out = np.zeros(cap, dense_normal_dtype)
        got = self._check(
            self.L.lsa_dense_map_get_normals(self.h, int(min_frames), float(max_miss_ratio), int(radius_leaves), int(min_neighbors), ptr(vp) if n else None, n, int(first_frame), ptr(out), cap),
            "lsa_dense_map_get_normals",
        )
        return out[:got].copy()

    def save_pcd_normals(self, path, fmt=PCD_BINARY, radius_leaves=2, min_neighbors=5, min_frames=1, max_miss_ratio=-1.0, viewpoints=None, first_frame=0):
        """the points of get(min_frames, max_miss_ratio) with the fields normal_x normal_y normal_z curvature of normals(...) behind
        them into a PCD file; returns their number (0 and no file for none)"""
        vp, n = _viewpoints(viewpoints)
        return self._check(
            self.L.lsa_dense_map_save_pcd_normals(
                self.h, os.fsencode(path), int(fmt), int(min_frames), float(max_miss_ratio), int(radius_leaves), int(min_neighbors), ptr(vp) if n else None, n, int(first_frame)
            ),
            "lsa_dense_map_save_pcd_normals",
        )

    def grid(self, cell_leaves=2, ground_radius=2, min_height=0.2, max_height=2.0, min_obstacle_voxels=1, min_frames=1, max_miss_ratio=-1.0, window=None):
        """(info, cells (height, width) dense_cell_dtype, state (height, width) int8) as DenseMapHost.grid states them, computed on
        the device from the table as it stands.  LsaError with .code E_ARG for what the statement refuses, E_CAPACITY for a
        grid of more than "GridMaxCells" cells; the map is untouched either way"""
        return _grid_call(lambda *a: self.L.lsa_dense_map_get_grid(self.h, *a), self._check, "lsa_dense_map_get_grid",
                          _grid_params(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, min_frames, max_miss_ratio, window))

    def save_grid(self, prefix, cell_leaves=2, ground_radius=2, min_height=0.2, max_height=2.0, min_obstacle_voxels=1, min_frames=1, max_miss_ratio=-1.0, window=None):
        """the states of grid(...) into <prefix>.pgm and <prefix>.yaml for map_server; returns the number of cells (0 and no
        files for none)"""
        p = _grid_params(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, min_frames, max_miss_ratio, window)
        return self._check(self.L.lsa_dense_map_save_grid(self.h, C.byref(p), os.fsencode(prefix)), "lsa_dense_map_save_grid")

    def cast(self, origins, targets, extend=0.0, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before=None):
        """(hits (n,) dense_hit_dtype, points (n,) LidarPoints) as DenseMapHost.cast states them, walked on the device: rays from
        origins ((n, 3) or (1, 3) float32) towards targets ((n, 3) float32).  LsaError with .code E_ARG for what the statement
        refuses; the map is untouched by the call"""
        tg = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
        org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        n = tg.shape[0]
        hits, points = np.zeros(max(n, 1), dense_hit_dtype), np.zeros(max(n, 1), POINT_DTYPE)
        p = _cast_params(extend, max_range, min_frames, max_miss_ratio, before)
        self._check(self.L.lsa_dense_map_cast(self.h, ptr(org) if org.size else ptr(np.zeros(3, np.float32)), org.shape[0], ptr(tg) if n else ptr(np.zeros(3, np.float32)), n,
                                              C.byref(p), ptr(hits), ptr(points)), "lsa_dense_map_cast")
        return hits[:n].copy(), points[:n].copy()

    def compare_points(self, points, origins, tolerance=None, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before=None):
        """(labels (n,) uint8, counts (4,) int64) as DenseMapHost.compare states them: world points of the caller's, every one
        from its origin ((n, 3) or (1, 3) float32); tolerance None: one leaf"""
        pts = np.ascontiguousarray(points, POINT_DTYPE)
        org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        labels, counts = np.zeros(max(pts.size, 1), np.uint8), np.zeros(4, np.int64)
        p = _cast_params(self.get_param("LeafSize") if tolerance is None else tolerance, max_range, min_frames, max_miss_ratio, before)
        self._check(self.L.lsa_dense_map_compare_points(self.h, ptr(pts) if pts.size else ptr(np.zeros(1, POINT_DTYPE)), pts.size,
                                                        ptr(org) if org.size else ptr(np.zeros(3, np.float32)), org.shape[0], C.byref(p), ptr(labels), ptr(counts)),
                    "lsa_dense_map_compare_points")
        return labels[:pts.size].copy(), counts

    def compare_frame(self, H0, H1=None, t0=0.0, t1=0.0, time_offset=0.0, tolerance=None, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before=None):
        """compare_points of the context's current frame moved as insert_frame moves it, every point from where the sensor stood
        at its time (frame_origins_at), fused with the walk: nothing of the frame leaves the device but the labels"""
        interp = H1 is not None
        cap = max(int(self.L.lsa_frame_size(self.ctx.h)), 1)
        labels, counts = np.zeros(cap, np.uint8), np.zeros(4, np.int64)
        p = _cast_params(self.get_param("LeafSize") if tolerance is None else tolerance, max_range, min_frames, max_miss_ratio, before)
        n = self._check(
            self.L.lsa_dense_map_compare_frame(self.h, int(interp), ptr(pose16(H0)), ptr(pose16(H1)) if interp else None, float(t0), float(t1), float(time_offset),
                                               C.byref(p), ptr(labels), cap, ptr(counts)),
            "lsa_dense_map_compare_frame",
        )
        return labels[:n].copy(), counts

    def save_pcd(self, path, fmt=PCD_BINARY, min_frames=1, max_miss_ratio=-1.0):
        """the points of get(min_frames, max_miss_ratio) into a PCD file; returns their number (0 and no file for none)"""
        return self._check(
            self.L.lsa_dense_map_save_pcd_filtered(self.h, os.fsencode(path), int(fmt), int(min_frames), float(max_miss_ratio)), "lsa_dense_map_save_pcd_filtered"
        )


def _cast_params(extend, max_range, min_frames, max_miss_ratio, before, use_before=None):
    """the lsa_dense_cast_params_t of a call (the library refuses what is out of range); before None: every voxel"""
    p = DenseCastParams()
    p.max_range, p.extend, p.max_miss_ratio = float(max_range), float(extend), float(max_miss_ratio)
    p.min_frames, p.before = int(min_frames), 0 if before is None else int(before)
    p.use_before = (0 if before is None else 1) if use_before is None else int(use_before)
    return p


def _viewpoints(viewpoints):
    """(float32 (n, 3) array or None, n); ValueError for another shape"""
    if viewpoints is None:
        return None, 0
    vp = np.asarray(viewpoints)
    if vp.ndim != 2 or vp.shape[1] != 3:
        raise ValueError("viewpoints of shape (n, 3)")
    vp = np.ascontiguousarray(vp, np.float32)
    return vp, vp.shape[0]


def _grid_params(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, min_frames, max_miss_ratio, window):
    """the lsa_dense_grid_params_t of a call; ValueError only for a window that is not four numbers (the library refuses the rest)"""
    p = DenseGridParams()
    p.cell_leaves, p.ground_radius, p.min_obstacle_voxels, p.min_frames = int(cell_leaves), int(ground_radius), int(min_obstacle_voxels), int(min_frames)
    p.min_height, p.max_height, p.max_miss_ratio = float(min_height), float(max_height), float(max_miss_ratio)
    if window is not None:
        w = np.asarray(window, np.float64).reshape(-1)
        if w.size != 4:
            raise ValueError("window = (x_min, y_min, x_max, y_max)")
        p.use_window = 1
        p.window[:] = w.tolist()
    return p


def _grid_call(call, check, what, p):
    """the two calls of a grid export: the extent alone (no output asked for: no cell is computed), then the cells"""
    info = DenseGridInfo()
    n = check(call(C.byref(p), C.byref(info), None, None, 0), what)
    cells, state = np.zeros(max(n, 1), dense_cell_dtype), np.zeros(max(n, 1), np.int8)
    if n > 0:
        n = check(call(C.byref(p), C.byref(info), ptr(cells), ptr(state), n), what)
    out = np.zeros((), dense_grid_info_dtype)
    for name in dense_grid_info_dtype.names:
        out[name] = getattr(info, name)
    h, w = int(info.height), int(info.width)
    return out, cells[:n].reshape(h, w).copy(), state[:n].reshape(h, w).copy()


def read_pcd_normals(path):
    """(n, 4) float32 normal_x normal_y normal_z curvature of a PCD file that has those fields, the bytes as the file holds them;
    LsaError naming the file when one is missing or is not a 4-byte F; host only"""
    L = lib()
    out = np.zeros((1, 4), np.float32)
    got = L.lsa_pcd_read_normals(os.fsencode(path), ptr(out), 0)
    if got > 0:
        out = np.zeros((got, 4), np.float32)
        got = L.lsa_pcd_read_normals(os.fsencode(path), ptr(out), got)
    if got < 0:
        raise LsaError(L.lsa_pcd_last_error().decode())
    return out[:got].copy()


def frame_origins_at(ctx, H0, H1=None, t0=0.0, t1=0.0, time_offset=0.0):
    """(n, 3) float32: where the sensor stood when it measured each point of the context's current frame -- the frame's own
    origin under the pose lsa_transform_frame_at gives the point: the origins of DenseMap.carve_frame"""
    n = ctx.L.lsa_frame_size(ctx.h)
    out = np.zeros((max(n, 1), 3), np.float32)
    interp = H1 is not None
    rc = ctx.L.lsa_transform_frame_origins_at(ctx.h, int(interp), ptr(pose16(H0)), ptr(pose16(H1)) if interp else None, float(t0), float(t1), float(time_offset), ptr(out), n)
    if rc < 0:
        raise _error("lsa_transform_frame_origins_at", rc, ctx.L.lsa_last_error(ctx.h).decode())
    return out[:rc].copy()


# ---- the pipeline's dense map (Slam.set_param("DenseMap", 1): every registered frame; 2: keyframes only)


def dense_map_size(slam):
    """voxels of the pipeline's dense map; waits for the insertions in flight.  LsaError (.code E_STATE) while "DenseMap" is 0"""
    return slam._check(slam.L.lsa_slam_dense_map_size(slam.h), "lsa_slam_dense_map_size")


def dense_map(slam, min_frames=1):
    """(points, voxels) of the pipeline's dense map with frames >= min_frames, in ascending key order"""
    cap = max(dense_map_size(slam), 1)
    pts, vox = np.zeros(cap, POINT_DTYPE), np.zeros(cap, dense_voxel_dtype)
    n = slam._check(slam.L.lsa_slam_get_dense_map(slam.h, int(min_frames), ptr(pts), ptr(vox), cap), "lsa_slam_get_dense_map")
    return pts[:n].copy(), vox[:n].copy()


def dense_map_sources(slam, min_frames=1):
    """int32 ordinals of the frames whose points the voxels of dense_map(slam, min_frames) hold, in its order"""
    cap = max(dense_map_size(slam), 1)
    out = np.zeros(cap, np.int32)
    n = slam._check(slam.L.lsa_slam_get_dense_map_sources(slam.h, int(min_frames), ptr(out), cap), "lsa_slam_get_dense_map_sources")
    return out[:n].copy()


def pose_corrections(old, new):
    """(n, 16) float64: new_i @ inverse(old_i) per pose, by the library's own arithmetic (lsa_pose_corrections) -- what
    Slam.set_trajectory hands the dense map's re-projection under "DenseMapOnTrajectory" 1"""
    a = np.ascontiguousarray(old, np.float64).reshape(-1, 16)
    b = np.ascontiguousarray(new, np.float64).reshape(-1, 16)
    if a.shape != b.shape:
        raise ValueError("as many new poses as old ones")
    out = np.zeros_like(a)
    rc = lib().lsa_pose_corrections(ptr(a), ptr(b), a.shape[0], ptr(out))
    if rc != 0:
        raise _error("lsa_pose_corrections", rc, "bad argument")
    return out


def save_dense_map_pcd(slam, path, format=PCD_BINARY, min_frames=1):  # noqa: A002 (the C ABI's name of the parameter)
    """the points of dense_map(slam, min_frames) into a PCD file; returns their number (0 and no file for none)"""
    return slam._check(slam.L.lsa_slam_save_dense_map_pcd(slam.h, os.fsencode(path), int(format), int(min_frames)), "lsa_slam_save_dense_map_pcd")


def dense_map_filtered(slam, min_frames=1, max_miss_ratio=-1.0):
    """dense_map of the voxels that also have misses <= max_miss_ratio * frames (a ratio below 0: all)"""
    cap = max(dense_map_size(slam), 1)
    pts, vox = np.zeros(cap, POINT_DTYPE), np.zeros(cap, dense_voxel_dtype)
    n = slam._check(slam.L.lsa_slam_get_dense_map_filtered(slam.h, int(min_frames), float(max_miss_ratio), ptr(pts), ptr(vox), cap), "lsa_slam_get_dense_map_filtered")
    return pts[:n].copy(), vox[:n].copy()


def dense_map_misses(slam, min_frames=1, max_miss_ratio=-1.0):
    """uint32 per voxel of dense_map_filtered(slam, min_frames, max_miss_ratio), in its order"""
    cap = max(dense_map_size(slam), 1)
    out = np.zeros(cap, np.uint32)
    n = slam._check(slam.L.lsa_slam_get_dense_map_misses(slam.h, int(min_frames), float(max_miss_ratio), ptr(out), cap), "lsa_slam_get_dense_map_misses")
    return out[:n].copy()


def prune_dense_map(slam, min_frames=1, max_miss_ratio=-1.0):
    """removes what dense_map_filtered leaves out from the pipeline's map; returns the number of voxels removed"""
    removed = C.c_longlong(0)
    slam._check(slam.L.lsa_slam_prune_dense_map(slam.h, int(min_frames), float(max_miss_ratio), C.byref(removed)), "lsa_slam_prune_dense_map")
    return int(removed.value)


def save_dense_map_pcd_filtered(slam, path, format=PCD_BINARY, min_frames=1, max_miss_ratio=-1.0):  # noqa: A002
    """the points of dense_map_filtered into a PCD file; returns their number (0 and no file for none)"""
    return slam._check(
        slam.L.lsa_slam_save_dense_map_pcd_filtered(slam.h, os.fsencode(path), int(format), int(min_frames), float(max_miss_ratio)), "lsa_slam_save_dense_map_pcd_filtered"
    )


def registered_frame_origins(slam):
    """(n, 3) float32 per point of slam.registered_frame(), in its order: where the sensor stood when it measured the point"""
    cap = max(slam._n, 1 << 19)  # as Slam.registered_frame
    out = np.zeros((cap, 3), np.float32)
    rc = slam._check(slam.L.lsa_slam_get_registered_frame_origins(slam.h, ptr(out), cap), "lsa_slam_get_registered_frame_origins")
    return out[:rc].copy()


def clear_dense_map(slam):
    slam._check(slam.L.lsa_slam_clear_dense_map(slam.h), "lsa_slam_clear_dense_map")


def dense_map_viewpoints(slam):
    """(viewpoints (n, 3) float32, first_frame): per inserted ordinal since the last clear where the sensor of the call's first
    frame stood -- the translation of its pose, narrowed to float, moved with the map by an applied trajectory under
    "DenseMapOnTrajectory" 1; first_frame is the ordinal of entry 0"""
    first = C.c_int(0)
    n = slam._check(slam.L.lsa_slam_get_dense_map_viewpoints(slam.h, None, 0, C.byref(first)), "lsa_slam_get_dense_map_viewpoints")
    out = np.zeros((max(n, 1), 3), np.float32)
    n = slam._check(slam.L.lsa_slam_get_dense_map_viewpoints(slam.h, ptr(out), out.shape[0], C.byref(first)), "lsa_slam_get_dense_map_viewpoints")
    return out[:n].copy(), int(first.value)


def dense_map_normals(slam, min_frames=1, max_miss_ratio=-1.0, radius_leaves=2, min_neighbors=5, orient=True):
    """dense_normal_dtype records of the voxels of dense_map_filtered(slam, min_frames, max_miss_ratio), in its order: DenseMap.normals
    of the pipeline's map, turned towards dense_map_viewpoints(slam) when `orient`"""
    cap = max(dense_map_size(slam), 1)
    out = np.zeros(cap, dense_normal_dtype)
    n = slam._check(
        slam.L.lsa_slam_get_dense_map_normals(slam.h, int(min_frames), float(max_miss_ratio), int(radius_leaves), int(min_neighbors), int(bool(orient)), ptr(out), cap),
        "lsa_slam_get_dense_map_normals",
    )
    return out[:n].copy()


def save_dense_map_pcd_normals(slam, path, format=PCD_BINARY, min_frames=1, max_miss_ratio=-1.0, radius_leaves=2, min_neighbors=5, orient=True):  # noqa: A002
    """dense_map_filtered with the normals of dense_map_normals behind every point into a PCD file; returns the number of points"""
    return slam._check(
        slam.L.lsa_slam_save_dense_map_pcd_normals(
            slam.h, os.fsencode(path), int(format), int(min_frames), float(max_miss_ratio), int(radius_leaves), int(min_neighbors), int(bool(orient))
        ),
        "lsa_slam_save_dense_map_pcd_normals",
    )


def dense_map_grid(slam, cell_leaves=2, ground_radius=2, min_height=0.2, max_height=2.0, min_obstacle_voxels=1, min_frames=1, max_miss_ratio=-1.0, window=None, half_extent=None):
    """DenseMap.grid of the pipeline's map: (info, cells, state).  half_extent (metres): the window of that half side around
    the translation of slam.world_transform() -- the local costmap -- when no window is given"""
    if window is None and half_extent is not None:
        T = np.asarray(slam.world_transform(), np.float64).reshape(4, 4)
        window = (T[0, 3] - float(half_extent), T[1, 3] - float(half_extent), T[0, 3] + float(half_extent), T[1, 3] + float(half_extent))
    return _grid_call(lambda *a: slam.L.lsa_slam_get_dense_map_grid(slam.h, *a), slam._check, "lsa_slam_get_dense_map_grid",
                      _grid_params(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, min_frames, max_miss_ratio, window))


def save_dense_map_grid(slam, prefix, cell_leaves=2, ground_radius=2, min_height=0.2, max_height=2.0, min_obstacle_voxels=1, min_frames=1, max_miss_ratio=-1.0, window=None):
    """the states of dense_map_grid into <prefix>.pgm and <prefix>.yaml; returns the number of cells (0 and no files for none)"""
    p = _grid_params(cell_leaves, ground_radius, min_height, max_height, min_obstacle_voxels, min_frames, max_miss_ratio, window)
    return slam._check(slam.L.lsa_slam_save_dense_map_grid(slam.h, C.byref(p), os.fsencode(prefix)), "lsa_slam_save_dense_map_grid")


# ---- rays through the pipeline's map (lsa_slam_cast_dense_map_rays, _render_dense_map_scan, _compare_frame_to_dense_map)


def dense_map_cast(slam, origins, targets, extend=0.0, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before=None):
    """DenseMap.cast of the pipeline's map: (hits, points).  LsaError (.code E_STATE) while "DenseMap" is 0"""
    tg = np.ascontiguousarray(targets, np.float32).reshape(-1, 3)
    org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    n = tg.shape[0]
    hits, points = np.zeros(max(n, 1), dense_hit_dtype), np.zeros(max(n, 1), POINT_DTYPE)
    p = _cast_params(extend, max_range, min_frames, max_miss_ratio, before)
    slam._check(slam.L.lsa_slam_cast_dense_map_rays(slam.h, ptr(org) if org.size else ptr(np.zeros(3, np.float32)), org.shape[0],
                                                    ptr(tg) if n else ptr(np.zeros(3, np.float32)), n, C.byref(p), ptr(hits), ptr(points)), "lsa_slam_cast_dense_map_rays")
    return hits[:n].copy(), points[:n].copy()


def dense_map_render_scan(slam, elevations, n_azimuth, pose=None, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before=None):
    """hits (n_rings, n_azimuth) dense_hit_dtype: the map as a spinning sensor of these ring elevations (radians) would see it
    from `pose` (4x4; None: where the sensor stands now, Tworld * BaseToLidarOffset) -- DenseMap.cast of scan_targets with
    extend = +inf, and nothing more.  hits["entry"] is the range image, status != 1 a ray that met nothing within max_range"""
    el = np.ascontiguousarray(elevations, np.float64).reshape(-1)
    n = el.size * int(n_azimuth)
    hits = np.zeros(max(n, 1), dense_hit_dtype)
    p = _cast_params(np.inf, max_range, min_frames, max_miss_ratio, before)
    slam._check(slam.L.lsa_slam_render_dense_map_scan(slam.h, ptr(pose16(pose)) if pose is not None else None, ptr(el) if el.size else ptr(np.zeros(1)), el.size, int(n_azimuth),
                                                      C.byref(p), ptr(hits)), "lsa_slam_render_dense_map_scan")
    return hits[:n].reshape(el.size, int(n_azimuth)).copy()


def dense_map_compare_frame(slam, tolerance=None, max_range=30.0, min_frames=1, max_miss_ratio=-1.0, before="auto"):
    """(labels uint8, counts (4,) int64): one label per point of slam.registered_frame(), in its order, as DenseMapHost.compare
    states them against the pipeline's map -- 2 (UNMAPPED) is a point the map does not know: the car that arrived.  tolerance
    None: one leaf.  before "auto": when the call that brought the current frame was inserted into the map, its ordinal -- the
    labels are against the map as it stood before this frame --, otherwise every voxel counts; None: every voxel; an ordinal:
    only voxels first seen before it.  Computed on the device from the frames it still holds; nothing is added to a frame"""
    cap = max(slam._n, 1 << 19)  # as Slam.registered_frame
    labels, counts = np.zeros(cap, np.uint8), np.zeros(4, np.int64)
    auto = isinstance(before, str)
    if auto and before != "auto":
        raise ValueError('before is "auto", None or an ordinal')
    p = _cast_params(float(slam.get_param("DenseMapLeafSize")) if tolerance is None else tolerance, max_range, min_frames, max_miss_ratio, None if auto else before,
                     use_before=2 if auto else None)
    n = slam._check(slam.L.lsa_slam_compare_frame_to_dense_map(slam.h, C.byref(p), ptr(labels), cap, ptr(counts)), "lsa_slam_compare_frame_to_dense_map")
    return labels[:n].copy(), counts
