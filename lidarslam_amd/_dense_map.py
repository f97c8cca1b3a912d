"""The dense point-cloud map: registered frames voxel-hashed on the device (lsa_dense_map_*, lsa_slam_*dense_map*).

DenseMapHost is the numpy statement of what the map computes; the device table (lidarslam_amd/csrc/lsa_dense_map.hip) is
held to it byte for byte, on points and voxel records.  DenseMap is the table alone on a Context; dense_map(slam, ...) and
its neighbours reach the pipeline's map (Slam.set_param("DenseMap", 1 or 2)).
"""
import ctypes as C
import os

import numpy as np

from ._abi import _error, lib
from ._native import POINT_DTYPE, pose16, ptr
from ._pcd import PCD_BINARY

# lsa_dense_voxel_t (include/lidarslam_amd.h)
dense_voxel_dtype = np.dtype([("key", "<u8"), ("count", "<u4"), ("frames", "<u4"), ("first_frame", "<i4"), ("last_frame", "<i4")])

DENSE_INDEX_RANGE = 1 << 20  # voxel indices lie in [-2^20, 2^20)


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
    surface voxels may merge, and the voxel between them may stay empty until it is seen again."""

    def __init__(self, leaf):
        if not (leaf > 0 and np.isfinite(leaf)):
            raise ValueError("leaf must be positive and finite")
        self.leaf = float(leaf)
        self.clear()

    def clear(self):
        self.voxels = {}
        self.skipped = 0
        self.dropped = 0
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
                self.voxels[key] = [pts[w].copy(), n, 1, frame, frame, c, frame]
                continue
            v[1] += n
            if v[4] != frame:
                v[2] += 1
                v[4] = frame
            if c > v[5]:
                v[0] = pts[w].copy()
                v[5] = c
                v[6] = frame

    def get(self, min_frames=1):
        """(points, voxels) of the voxels with frames >= min_frames, in ascending key order"""
        keys = sorted(k for k, v in self.voxels.items() if v[2] >= min_frames)
        pts = np.zeros(len(keys), POINT_DTYPE)
        vox = np.zeros(len(keys), dense_voxel_dtype)
        for j, k in enumerate(keys):
            p, count, frames, first, last = self.voxels[k][:5]
            pts[j] = p
            vox[j] = (k, count, frames, first, last)
        return pts, vox

    def sources(self, min_frames=1):
        """the source of every voxel of get(min_frames), in its order"""
        keys = sorted(k for k, v in self.voxels.items() if v[2] >= min_frames)
        return np.array([self.voxels[k][6] for k in keys], np.int32)

    def reproject(self, corrections, first_frame=0):
        """corrections: (n, 16) float64, row-major 4x4 rigid transforms, entry j for ordinal first_frame + j.  Returns the
        number of voxels dropped (also added to self.dropped; skipped is not touched).

        Every voxel takes entry c = clamp(source - first_frame, 0, n - 1) and its point moves as rigid_apply of
        lsa_device_math.h moves it, in double, without contraction, narrowed to float: x' = (float)(((R0*x + R1*y) + R2*z)
        + t0), likewise y' and z' (so a -0.0 comes out +0.0 under the identity); the other 20 bytes are kept.  The new key
        is dense_voxel_keys of the moved point; a moved point that is not finite or lies outside the index range drops its
        voxel.  Voxels that arrive at one key merge: count is the sum modulo 2^32, first_frame the min, last_frame the
        max, frames = min(sum of frames, last_frame - first_frame + 1), point and source from the voxel of largest
        intensity code, ties to the smaller source, then to the smaller old key.  Nothing depends on the order in which
        the voxels are visited; last_frame of the map, the guard on the ordinals, is unchanged."""
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
            p, count, frames, first, last, code, src = recs[j]
            rank = (-code, src, old[j])  # the smallest wins: largest code, then smaller source, then smaller old key
            m = merged.get(int(keys[j]))
            if m is None:
                merged[int(keys[j])] = [pts[j].copy(), count, frames, first, last, code, src, rank]
                continue
            m[1] = (m[1] + count) & 0xFFFFFFFF
            m[2] += frames
            m[3], m[4] = min(m[3], first), max(m[4], last)
            if rank < m[7]:
                m[0], m[5], m[6], m[7] = pts[j].copy(), code, src, rank
        self.voxels = {k: [m[0], m[1], min(m[2], m[4] - m[3] + 1), m[3], m[4], m[5], m[6]] for k, m in merged.items()}
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

    def get(self, min_frames=1):
        """(points, voxels) with frames >= min_frames in ascending key order"""
        cap = max(self.size(), 1)
        pts, vox = np.zeros(cap, POINT_DTYPE), np.zeros(cap, dense_voxel_dtype)
        n = self._check(self.L.lsa_dense_map_get(self.h, int(min_frames), ptr(pts), ptr(vox), cap), "lsa_dense_map_get")
        return pts[:n].copy(), vox[:n].copy()

    def sources(self, min_frames=1):
        """int32 ordinals of the calls whose points the voxels of get(min_frames) hold, in its order"""
        cap = max(self.size(), 1)
        out = np.zeros(cap, np.int32)
        n = self._check(self.L.lsa_dense_map_get_sources(self.h, int(min_frames), ptr(out), cap), "lsa_dense_map_get_sources")
        return out[:n].copy()

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

    def save_pcd(self, path, fmt=PCD_BINARY, min_frames=1):
        """the points of get(min_frames) into a PCD file; returns their number (0 and no file for none)"""
        return self._check(self.L.lsa_dense_map_save_pcd(self.h, os.fsencode(path), int(fmt), int(min_frames)), "lsa_dense_map_save_pcd")


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


def clear_dense_map(slam):
    slam._check(slam.L.lsa_slam_clear_dense_map(slam.h), "lsa_slam_clear_dense_map")
