"""PCD files and the LZF codec; host only."""
import ctypes as C
import os

import numpy as np

from ._abi import LsaError, lib
from ._native import POINT_DTYPE, ptr

PCD_ASCII, PCD_BINARY, PCD_BINARY_COMPRESSED = 0, 1, 2  # PCDFormat (PointCloudStorage.h:60-65)
PCD_FORMAT_NAMES = ["ascii", "binary", "binary_compressed"]


def pcd_info(path):
    """(number of points, format) of a PCD file; host only"""
    L = lib()
    n, fmt = C.c_int(), C.c_int()
    if L.lsa_pcd_info(os.fsencode(path), C.byref(n), C.byref(fmt)) != 0:
        raise LsaError(L.lsa_pcd_last_error().decode())
    return n.value, fmt.value


def read_pcd(path):
    """A PCD file as LidarPoints (POINT_DTYPE): any field order, missing fields 0, extra fields ignored; host only."""
    L = lib()
    n, _ = pcd_info(path)
    out = np.zeros(max(n, 1), POINT_DTYPE)
    got = L.lsa_pcd_read(os.fsencode(path), ptr(out), out.size)
    if got < 0:
        raise LsaError(L.lsa_pcd_last_error().decode())
    return out[:got].copy()


def write_pcd(path, pts, fmt=PCD_BINARY):
    """Writes LidarPoints as a PCD file (fmt: 0 ascii, 1 binary, 2 binary_compressed); host only.  Returns False, and
    writes nothing, for an empty cloud (savePointCloudToPCD's -3)."""
    L = lib()
    pts = np.ascontiguousarray(pts, POINT_DTYPE)
    rc = L.lsa_pcd_write(os.fsencode(path), ptr(pts) if pts.size else None, pts.size, int(fmt))
    if rc == -3 and pts.size == 0:
        return False
    if rc != 0:
        raise LsaError(f"lsa_pcd_write failed ({rc}): {L.lsa_pcd_last_error().decode()}")
    return True


def lzf_compress(data):
    L = lib()
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.zeros(src.size + src.size // 16 + 64, np.uint8)
    n = C.c_size_t()
    if L.lsa_lzf_compress(ptr(src) if src.size else None, src.size, ptr(out), out.size, C.byref(n)) != 0:
        raise LsaError("lsa_lzf_compress failed")
    return out[: n.value].tobytes()


def lzf_decompress(data, raw_size):
    L = lib()
    src = np.frombuffer(bytes(data), np.uint8)
    out = np.zeros(max(raw_size, 1), np.uint8)
    n = C.c_size_t()
    if L.lsa_lzf_decompress(ptr(src) if src.size else None, src.size, ptr(out), raw_size, C.byref(n)) != 0:
        raise LsaError("lsa_lzf_decompress: malformed stream")
    return out[: n.value].tobytes()
