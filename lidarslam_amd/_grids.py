"""The rolling voxel maps: RollingGrid on the host, DeviceGrid in a context's memory."""
import ctypes as C
import os

import numpy as np

from ._abi import TARGET_MAP, LsaError, lib
from ._native import PLANE, POINT_DTYPE, pose16, ptr
from ._pcd import PCD_BINARY


class RollingGrid:
    """LidarSlam::RollingGrid (RollingGrid.h:63-212) as the pipeline uses it: host code, no device involved."""

    def __init__(self, **params):
        self.L = lib()
        self.h = C.c_void_p(self.L.lsa_rolling_grid_create())
        if not self.h:
            raise LsaError("lsa_rolling_grid_create failed")
        for k, v in params.items():
            self.set(k, v)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.lsa_rolling_grid_destroy(self.h)
            self.h = None

    def set(self, name, value):
        if self.L.lsa_rolling_grid_set(self.h, name.encode(), float(value)) != 0:
            raise LsaError(f"lsa_rolling_grid_set({name}, {value}) refused")

    def reset(self, position=None):
        pos = None if position is None else np.ascontiguousarray(position, np.float32)
        self.L.lsa_rolling_grid_reset(self.h, None if pos is None else ptr(pos))

    def clear(self):
        self.L.lsa_rolling_grid_clear(self.h)

    def size(self):
        return self.L.lsa_rolling_grid_size(self.h)

    def roll(self, mn, mx):
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        self.L.lsa_rolling_grid_roll(self.h, ptr(mn), ptr(mx))

    def add(self, pts, fixed=False, time=-1.0, roll=True):
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        if self.L.lsa_rolling_grid_add(self.h, ptr(pts) if pts.size else None, pts.size, int(fixed), float(time), int(roll)) != 0:
            raise LsaError("lsa_rolling_grid_add failed")

    def clear_old_points(self, time):
        self.L.lsa_rolling_grid_clear_old_points(self.h, float(time))

    def get(self, clean=False):
        out = np.zeros(max(self.size(), 1), POINT_DTYPE)
        n = self.L.lsa_rolling_grid_get(self.h, int(clean), ptr(out), out.size)
        return out[:n].copy()

    def build_submap(self, mn=None, mx=None, min_nb_points=-1):
        if mn is None:
            return self.L.lsa_rolling_grid_build_submap(self.h, None, None, -1)
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        return self.L.lsa_rolling_grid_build_submap(self.h, ptr(mn), ptr(mx), int(min_nb_points))

    def submap_valid(self):
        return bool(self.L.lsa_rolling_grid_submap_valid(self.h))

    def submap(self):
        out = np.zeros(max(self.size(), 1), POINT_DTYPE)
        n = self.L.lsa_rolling_grid_submap(self.h, ptr(out), out.size)
        return out[:n].copy()


class DeviceGrid:
    """LidarSlam::RollingGrid resident on the device (lsa_device_grid_*): same calls as RollingGrid, the map lives in the
    memory of `ctx` and its sub-map becomes a kNN target of that context."""

    def __init__(self, ctx, **params):
        self.L = lib()
        self.ctx = ctx
        h = C.c_void_p()
        if self.L.lsa_device_grid_create(ctx.h, C.byref(h)) != 0:
            raise LsaError("lsa_device_grid_create failed")
        self.h = h
        for k, v in params.items():
            self.set(k, v)

    def close(self):
        if getattr(self, "h", None):
            if self.ctx.h:  # a grid must go before its context (include/lidarslam_amd.h); one that outlived it is dropped
                self.L.lsa_device_grid_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc < 0:
            raise LsaError(f"{what} failed ({rc}): {self.L.lsa_last_error(self.ctx.h).decode()}")
        return rc

    def set(self, name, value):
        self._check(self.L.lsa_device_grid_set(self.h, name.encode(), float(value)), f"lsa_device_grid_set({name})")

    def get_param(self, name):
        return float(self.L.lsa_device_grid_get_param(self.h, name.encode()))

    def reset(self, position=None):
        pos = None if position is None else np.ascontiguousarray(position, np.float32)
        self._check(self.L.lsa_device_grid_reset(self.h, None if pos is None else ptr(pos)), "lsa_device_grid_reset")

    def clear(self):
        self._check(self.L.lsa_device_grid_clear(self.h), "lsa_device_grid_clear")

    def size(self):
        return self._check(self.L.lsa_device_grid_size(self.h), "lsa_device_grid_size")

    def roll(self, mn, mx):
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        self._check(self.L.lsa_device_grid_roll(self.h, ptr(mn), ptr(mx)), "lsa_device_grid_roll")

    def add(self, pts, fixed=False, time=-1.0, roll=True):
        pts = np.ascontiguousarray(pts, POINT_DTYPE)
        self._check(self.L.lsa_device_grid_add(self.h, ptr(pts) if pts.size else None, pts.size, int(fixed), float(time), int(roll)), "lsa_device_grid_add")

    def add_keypoints(self, kset, ktype, pose, time):
        self._check(self.L.lsa_device_grid_add_keypoints(self.h, kset, ktype, ptr(pose16(pose)), float(time)), "lsa_device_grid_add_keypoints")

    def stage_keypoints(self, kset, ktype, pose):
        self._check(self.L.lsa_device_grid_stage_keypoints(self.h, kset, ktype, ptr(pose16(pose))), "lsa_device_grid_stage_keypoints")

    def add_staged(self, time):
        """the insertion of what stage_keypoints read; any host thread"""
        self._check(self.L.lsa_device_grid_add_staged(self.h, float(time)), "lsa_device_grid_add_staged")

    def add_pcd(self, path, fixed=False, time=-1.0, roll=True):
        """RollingGrid::Add of a PCD file's cloud, converted on the device"""
        self._check(self.L.lsa_device_grid_add_pcd(self.h, os.fsencode(path), int(fixed), float(time), int(roll)), "lsa_device_grid_add_pcd")

    def save_pcd(self, path, fmt=PCD_BINARY, clean=False):
        """RollingGrid::Get(clean) into a PCD file; returns the points written (0 and no file for an empty map)"""
        return self._check(self.L.lsa_device_grid_save_pcd(self.h, os.fsencode(path), int(fmt), int(clean)), "lsa_device_grid_save_pcd")

    def pcd_io_times(self):
        o = np.zeros(8)
        self.L.lsa_pcd_io_times(self.ctx.h, ptr(o))
        return o

    def build_submap_begin_for_keypoints(self, box_type, min_nb_points, ktype=PLANE, slot=TARGET_MAP):
        """box of the keypoints of `box_type` as Context.keypoint_bboxes_begin left it on the device"""
        self._check(self.L.lsa_device_grid_build_submap_begin_for_keypoints(self.h, box_type, int(min_nb_points), slot, ktype), "lsa_device_grid_build_submap_begin_for_keypoints")

    def build_submap_end(self):
        return self._check(self.L.lsa_device_grid_build_submap_end(self.h), "lsa_device_grid_build_submap_end")

    def submap_ahead_begin(self, box_type, min_nb_points, ktype=PLANE):
        """the sub-map for the box Context.keypoint_bboxes_begin left on the device, ahead of time, into the spare target"""
        self._check(self.L.lsa_device_grid_submap_ahead_begin(self.h, box_type, int(min_nb_points), ktype), "lsa_device_grid_submap_ahead_begin")

    def submap_ahead_wait(self):
        return self._check(self.L.lsa_device_grid_submap_ahead_wait(self.h), "lsa_device_grid_submap_ahead_wait")

    def submap_ahead_take(self, box_type, min_nb_points, ktype=PLANE, slot=TARGET_MAP):
        """(size, taken): taken == 1 when the sub-map extracted ahead became target (slot, ktype)"""
        taken = C.c_int(0)
        n = self._check(self.L.lsa_device_grid_submap_ahead_take(self.h, box_type, int(min_nb_points), slot, ktype, C.byref(taken)), "lsa_device_grid_submap_ahead_take")
        return n, taken.value

    def clear_old_points(self, time):
        self._check(self.L.lsa_device_grid_clear_old_points(self.h, float(time)), "lsa_device_grid_clear_old_points")

    def get(self, clean=False, capacity=None):
        """RollingGrid::Get(clean); capacity: room for so many points (default: the voxels the map holds)"""
        if capacity is None:
            capacity = max(int(self.get_param("Voxels")), 1)
        out = np.zeros(capacity, POINT_DTYPE)
        n = self._check(self.L.lsa_device_grid_get(self.h, int(clean), ptr(out), out.size), "lsa_device_grid_get")
        return out[:n].copy()

    def build_submap(self, mn=None, mx=None, min_nb_points=-1, ktype=PLANE, slot=TARGET_MAP):
        """the sub-map becomes target (slot, ktype) of the context; returns its size"""
        if mn is None:
            return self._check(self.L.lsa_device_grid_build_submap(self.h, None, None, -1, slot, ktype), "lsa_device_grid_build_submap")
        mn, mx = np.ascontiguousarray(mn, np.float32), np.ascontiguousarray(mx, np.float32)
        return self._check(self.L.lsa_device_grid_build_submap(self.h, ptr(mn), ptr(mx), int(min_nb_points), slot, ktype), "lsa_device_grid_build_submap")

    def submap_valid(self):
        return bool(self.L.lsa_device_grid_submap_valid(self.h))
