"""DenseMapHost.cast and .compare, the definition of the dense map's rays (lidarslam_amd/_dense_map.py): the walk that stops at
the first voxel that counts, the record, the predicate, the labels, and an independent statement by slabs.  Numpy alone: no GPU
(the native library only where a test says so).  Cases: tests/dense_cast_cases.py."""
import os

import numpy as np
import pytest

import dense_carve_cases as K
import dense_cast_cases as R
from lidarslam_amd._dense_map import DenseMapHost, _scan_targets_numpy, dense_hit_dtype, scan_targets
from lidarslam_amd._native import LIB_PATH

LEAF = K.LEAF


def one(h, o, t, **kw):
    hits, points = h.cast(o, t, **kw)
    assert hits.dtype == dense_hit_dtype and hits.dtype.itemsize == 32 and len(hits) == len(points) == 1
    return hits[0], points[0]


def zero_but(hit, point, steps, status):
    assert (int(hit["steps"]), int(hit["status"])) == (steps, status)
    assert int(hit["key"]) == 0 and hit["entry"] == hit["exit"] == hit["depth"] == 0 and int(hit["source"]) == 0 and point.tobytes() == bytes(32)


# ---- the walk -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.RAY_CASES))
def test_every_ray_case_on_an_empty_map_at_its_end_and_past_it(name):
    o, t, kw = R.cast_case(name)
    visited = K.walk(name)
    assert (visited is None) == (name in K.NO_RAY)
    hit, point = one(DenseMapHost(LEAF), o, t, **kw)
    if visited is None:
        zero_but(hit, point, 0, -1)  # under_margin / at_margin: tt not > 0 under the negative extend
        return
    zero_but(hit, point, len(visited), 0)
    mine = R.cast_walks(o, t, **kw)[0]
    assert [v for v, _, _ in mine] == visited  # the carve's walk
    tt = min(float(np.linalg.norm(t[0].astype(np.float64) - o[0].astype(np.float64))) + kw["extend"], kw["max_range"])
    # a voxel at the last index of the walk is hit, with the whole walk behind it; its exit is the ray's end
    h = R.host_with([visited[-1]], frame=3)
    hit, point = one(h, o, t, **kw)
    assert (int(hit["status"]), int(hit["steps"]), int(hit["key"]), int(hit["source"])) == (1, len(visited), R.key_of(visited[-1]), 3)
    assert point.tobytes() == h.get()[0][0].tobytes()
    assert hit["entry"] <= hit["exit"] and hit["exit"] == np.float32(np.float64(mine[-1][2]) * tt) and mine[-1][2] == 1.0
    assert abs(float(hit["exit"]) - tt) <= 1e-6 * tt  # (float)tt up to the double product's rounding
    assert hit["entry"] == np.float32(mine[-1][1] * tt)
    # one voxel past the end is not
    if len(visited) > 1:
        past = tuple(2 * a - b for a, b in zip(visited[-1], visited[-2]))
        if all(-(1 << 20) <= v < (1 << 20) for v in past):
            zero_but(*one(R.host_with([past]), o, t, **kw), len(visited), 0)


@pytest.mark.parametrize("name", sorted(K.TIES))
def test_a_tie_is_hit_in_the_written_out_order(name):
    o, t, kw = R.cast_case(name)
    visited = K.TIES[name]
    assert K.walk(name) == visited
    for k in range(len(visited) - 1):
        here, there = np.array(visited[k]), np.array(visited[k + 1])
        toward = np.sign(np.array(visited[-1]) - here)
        others = [tuple(here + toward * np.eye(3, dtype=np.int64)[a]) for a in range(3) if toward[a] != 0]
        assert tuple(there) in others
        hit, _ = one(R.host_with(others), o, t, **kw)  # voxels at every candidate of the step: the one the walk visits first
        assert (int(hit["status"]), int(hit["steps"]), int(hit["key"])) == (1, k + 2, R.key_of(there)), (name, k)


def test_the_start_voxel_occupied():
    o, t, kw = R.cast_case("through_zero")
    visited = K.walk("through_zero")
    hit, _ = one(R.host_with(visited), o, t, **kw)
    assert (int(hit["status"]), int(hit["steps"]), int(hit["key"])) == (1, 1, R.key_of(visited[0])) and hit["entry"] == 0 and hit["exit"] > 0


def test_entry_and_exit_run_along_the_ray():
    o, t, kw = R.cast_case("long")
    walk = R.cast_walks(o, t, **kw)[0]
    assert walk[0][1] == 0.0 and walk[-1][2] == 1.0
    for (_, a, b), (_, a2, _) in zip(walk, walk[1:]):
        assert a <= b and a2 == b  # a voxel is entered where the one before was left
    for k in (1, len(walk) // 2, len(walk) - 2):
        hit, _ = one(R.host_with([walk[k][0]]), o, t, **kw)
        assert int(hit["steps"]) == k + 1 and hit["entry"] == np.float32(walk[k][1] * 30.0) and hit["exit"] == np.float32(walk[k][2] * 30.0) and hit["entry"] < hit["exit"]


def test_extend_moves_the_end_and_infinity_runs_to_the_range():
    o, t = np.array([[0.125, 0.125, 0.125]], np.float32), np.array([[3.125, 0.125, 0.125]], np.float32)
    steps = {e: int(one(DenseMapHost(LEAF), o, t, extend=e, max_range=10.0)[0]["steps"]) for e in R.EXTENDS}
    assert steps == {0.0: 7, LEAF: 8, float("inf"): 21, -2.0 * LEAF: 5}  # ends at x = 3.125, 3.625, 10.125, 2.125
    with pytest.raises(ValueError):
        DenseMapHost(LEAF).cast(o, t, extend=float("nan"))
    for bad in (0.0, -1.0, float("inf"), 4096 * LEAF * 1.001):
        with pytest.raises(ValueError):
            DenseMapHost(LEAF).cast(o, t, max_range=bad)
    with pytest.raises(ValueError):
        DenseMapHost(LEAF).cast(o, t, min_frames=0)
    zero_but(*one(DenseMapHost(LEAF), o, o), 0, -1)  # len 0: no ray, also under a positive extend
    zero_but(*one(DenseMapHost(LEAF), o, o, extend=1.0), 0, -1)


# ---- the predicate ------------------------------------------------------------------------------------------------------------
def test_a_voxel_that_fails_a_part_of_the_predicate_is_walked_through():
    o, t, kw = R.cast_case("axis+x")
    kw["extend"] = 0.0
    first, second = (2, 0, 0), (4, 0, 0)
    h = DenseMapHost(LEAF)
    h.insert(K.voxel_points([second]), 0)
    h.insert(K.voxel_points([second]), 1)
    h.insert(K.voxel_points([first]), 2)  # seen once, from ordinal 2 on
    key = lambda **more: int(one(h, o, t, **kw, **more)[0]["key"])  # noqa: E731
    assert key() == R.key_of(first) and key(min_frames=2) == R.key_of(second) and key(before=2) == R.key_of(second) and key(before=3) == R.key_of(first)
    zero_but(*one(h, o, t, **kw, before=0), 7, 0)
    # after a carve through both: `first` is seen through in ordinal 3 (1 miss of 1 frame), `second` was hit in it
    far = K.voxel_points([second])
    h.insert(far, 3)
    h.carve(far, o, 3, margin_leaves=0.0)
    assert h.misses().tolist() == [1, 0]
    assert key(max_miss_ratio=0.5) == R.key_of(second) and key(max_miss_ratio=1.0) == R.key_of(first) and key(max_miss_ratio=-1.0) == R.key_of(first)


# ---- the independent statement ------------------------------------------------------------------------------------------------
def test_the_hit_is_the_occupied_voxel_of_smallest_slab_entry():
    rng = np.random.default_rng(11)
    origins = rng.uniform(-1, 1, (2000, 3)).astype(np.float32)
    targets = rng.uniform(-6, 6, (2000, 3)).astype(np.float32)
    voxels = np.unique(rng.integers(-12, 13, (900, 3)), axis=0)
    h = R.host_with(voxels)
    before = R.state(h)
    hits, _ = h.cast(origins, targets, extend=0.0)
    first, left_out = R.slab_first_hits(origins, targets, voxels, LEAF)
    expected = np.where(first >= 0, np.array([R.key_of(v) for v in voxels], np.uint64)[np.maximum(first, 0)], np.uint64(0))
    print("hits", int((hits["status"] == 1).sum()), "left out", int(left_out.sum()), "wrong", int(((hits["key"] != expected) & ~left_out).sum()))
    assert left_out.sum() <= 0.01 * len(left_out)  # a condition of the check, not a finding
    assert (hits["status"] >= 0).all() and (hits["status"] == 1).sum() > 1000
    assert ((hits["key"] == expected) | left_out).all() and (((hits["status"] == 1) == (first >= 0)) | left_out).all()
    assert (hits["entry"] <= hits["exit"]).all()
    assert R.state(h) == before and h.cast_rays == 2000


# ---- compare ------------------------------------------------------------------------------------------------------------------
def test_compare_on_the_wall():
    h, wall = R.wall_only()
    before = R.state(h)
    labels, counts = h.compare(wall, K.SENSOR)  # tolerance: one leaf
    assert labels.dtype == np.uint8 and set(labels.tolist()) <= {h.CONSISTENT, h.THROUGH_MAP} and (labels == h.CONSISTENT).sum() > 0
    assert counts.tolist() == np.bincount(labels, minlength=4).tolist() and counts.sum() == len(wall)
    probes = K.cloud([R.IN_FRONT, R.BEHIND, R.BEYOND])
    labels, counts = h.compare(probes, K.SENSOR)
    assert labels.tolist() == [h.UNMAPPED, h.THROUGH_MAP, h.NOT_JUDGED] and counts.tolist() == [1, 0, 1, 1]
    per_point = np.repeat(K.SENSOR, 3, axis=0)
    assert h.compare(probes, per_point)[0].tolist() == labels.tolist()
    # a point in the wall's own voxel is consistent at any tolerance; the wall as it stood before ordinal 0 is no wall
    assert h.compare(wall[84:85], K.SENSOR, tolerance=0.0)[0].tolist() == [h.CONSISTENT]
    assert h.compare(wall, K.SENSOR, before=0)[1].tolist() == [0, 0, len(wall), 0]
    bad = K.cloud([(np.nan, 0, 0)])
    assert h.compare(bad, K.SENSOR)[0].tolist() == [h.NOT_JUDGED]
    for tolerance in (-0.1, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            h.compare(wall, K.SENSOR, tolerance=tolerance)
    assert R.state(h) == before and h.cast_rays == 2 * len(wall) + 3 + 3 + 1  # (the NaN point casts none)


def test_the_carved_scene_before_and_after_the_object_left():
    h, wall, obj = K.host_scene()
    before = R.state(h)
    wall_pts = K.voxel_points(wall)
    everything = h.compare(wall_pts, K.SENSOR)[0]
    seen = h.compare(wall_pts, K.SENSOR, max_miss_ratio=0.5)[0]  # the object's voxels were seen through more often than seen
    assert (everything == h.THROUGH_MAP).sum() > (seen == h.THROUGH_MAP).sum() and set(seen.tolist()) <= {h.CONSISTENT, h.THROUGH_MAP}
    assert R.state(h) == before


# ---- scan targets -------------------------------------------------------------------------------------------------------------
def test_scan_targets_are_ring_major_from_the_poses_x_axis():
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]  # the sensor's x axis is the world's y
    T[:3, 3] = [1.5, -2.0, 0.25]
    el = np.deg2rad([-15.0, 0.0, 10.0])
    origin, targets = _scan_targets_numpy(T, el, 8)
    assert origin.dtype == targets.dtype == np.float32 and origin.shape == (1, 3) and targets.shape == (24, 3)
    assert origin.tolist() == [[1.5, -2.0, 0.25]]
    grid = targets.reshape(3, 8, 3).astype(np.float64) - T[:3, 3]
    assert np.allclose(grid[1, 0], [0, 1, 0], atol=1e-6) and np.allclose(grid[1, 2], [-1, 0, 0], atol=1e-6)  # az_0 along x, az_2 a quarter turn on
    assert np.allclose(grid[:, :, 2], np.sin(el)[:, None], atol=1e-6) and np.allclose(np.linalg.norm(grid, axis=2), 1.0, atol=1e-6)
    if os.path.exists(LIB_PATH):
        # scan_targets hands out the C function's floats, to the byte
        import lidarslam_amd as L

        co, ct = np.zeros((1, 3), np.float32), np.zeros((24, 3), np.float32)
        assert L.lib().lsa_scan_targets(L.ptr(L.pose16(T)), L.ptr(np.ascontiguousarray(el, np.float64)), 3, 8, L.ptr(co), L.ptr(ct)) == 0
        o2, t2 = scan_targets(T, el, 8)
        assert o2.tobytes() == co.tobytes() == origin.tobytes() and t2.tobytes() == ct.tobytes()
        # the numpy statement beside them: numpy's cos and sin may differ from the C library's in the last bit of the double,
        # which can move a float by one unit in the last place -- 2.4e-7 at these magnitudes (below 4); hence 1e-6 and not bytes
        assert np.abs(t2 - targets).max() <= 1e-6
        big = scan_targets(T, np.deg2rad(np.linspace(-15, 15, 16)), 360)[1]
        assert big.shape == (16 * 360, 3) and scan_targets(T, [], 360)[1].shape == (0, 3)


# ---- the structs against the compiler ----------------------------------------------------------------------------------------
def test_the_cast_structs_have_the_compilers_layout(tmp_path):
    """lsa_dense_cast_params_t and lsa_dense_hit_t as g++ lays them out against DenseCastParams and dense_hit_dtype, as
    tests/test_abi.py holds the other mirrors"""
    import ctypes as C
    import shutil
    import subprocess

    from lidarslam_amd._dense_map import DenseCastParams

    if shutil.which("g++") is None:
        pytest.skip("no g++ to lay the header's structs out")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mirrors = {
        "lsa_dense_cast_params_t": (C.sizeof(DenseCastParams), {f[0]: (getattr(DenseCastParams, f[0]).offset, getattr(DenseCastParams, f[0]).size) for f in DenseCastParams._fields_}),
        "lsa_dense_hit_t": (dense_hit_dtype.itemsize, {f: (dense_hit_dtype.fields[f][1], dense_hit_dtype.fields[f][0].itemsize) for f in dense_hit_dtype.names}),
    }
    assert mirrors["lsa_dense_cast_params_t"][0] == 40 and mirrors["lsa_dense_hit_t"][0] == 32
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "lidarslam_amd.h"', "int main()", "{"]
    for c, (_, fields) in mirrors.items():
        lines.append(f'  std::printf("{c} . 0 %zu\\n", sizeof({c}));')
        lines += [f'  std::printf("{c} {f} %zu %zu\\n", offsetof({c}, {f}), sizeof((({c}*)0)->{f}));' for f in fields]
    lines += ["  return 0;", "}", ""]
    (tmp_path / "layout.cpp").write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-invalid-offsetof", "-I" + os.path.join(root, "include"), str(tmp_path / "layout.cpp"), "-o", exe])
    compiled = {}
    for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines():
        c, f, offset, size = line.split()
        compiled.setdefault(c, [0, {}])
        if f == ".":
            compiled[c][0] = int(size)
        else:
            compiled[c][1][f] = (int(offset), int(size))
    for c, (size, fields) in mirrors.items():
        assert (size, fields) == tuple(compiled[c]), c
