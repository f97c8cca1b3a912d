"""The dense map's normals on the device (lidarslam_amd/csrc/lsa_dense_normals.hip: k_dense_normals) against the host statement
(DenseMapHost.normals with the oracle's eigen33 as the eigen step), on the bytes of all 20 of every record, the NaN of "no
normal" included: the cases of tests/dense_normals_cases.py, group and wavefront edges, long probe sequences, the smallest
table, the map after growth, re-projection, carving, pruning and a clear, refusals, the pipeline, files."""
import os

import numpy as np
import pytest

import dense_carve_cases as K
import dense_map_cases as M
import dense_normals_cases as N
from conftest import two_device_rig

pytestmark = pytest.mark.gpu

PIPE_LEAF = 0.2


@pytest.fixture(scope="module")
def eig(O):
    return lambda cov: O.numerics(3, cov)


def same_normals(d, h, eig, **q):
    """the device's records of query q are the host's, byte for byte; returns them"""
    want = h.normals(eig=eig, **q)
    got = d.normals(**q)
    assert got.dtype == want.dtype and got.dtype.itemsize == 20 and len(got) == len(want)
    assert got["neighbors"].tobytes() == want["neighbors"].tobytes()
    assert got.tobytes() == want.tobytes(), int((N.float_bits(got) != N.float_bits(want)).any(axis=1).sum())
    return got


def pair(L, ctx, leaf, steps, **params):
    d = N.play(L.DenseMap(ctx, leaf, **params), steps)
    h = N.play(L.DenseMapHost(leaf), steps)
    return d, h


# ---- the cases of the definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(N.CASES))
def test_every_case_and_query(L, gpu_ctx, eig, name):
    leaf, steps, queries, params = N.CASES[name]()
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    assert K.same_state(d, h) == h.size() > 0
    fitted = 0
    for q in queries:
        fitted += int((~N.no_normal(same_normals(d, h, eig, **q))).sum())
    assert (fitted > 0) == (name != "lone")
    assert K.same_state(d, h) == h.size()  # read-only
    d.close()


@pytest.mark.parametrize("n", N.COUNTS)
def test_exported_counts_at_group_and_wavefront_edges(L, gpu_ctx, eig, n):
    leaf, steps, queries, params = N.counted(n)
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    assert d.size() == 2 * n and len(h.get(2)[1]) == n  # the exported list is sparser than the table
    for q in queries:
        got = same_normals(d, h, eig, **q)
        assert len(got) == (n if q.get("min_frames") == 2 else 2 * n)
    d.close()


def test_probe_stress_and_the_smallest_table(L, gpu_ctx, eig):
    pts = M.distinct_voxels(300, seed=6)
    d, h = pair(L, gpu_ctx, M.LEAF, [("insert", pts[:200], 0), ("insert", pts[100:], 1)], InitialCapacity=64, ProbeStress=1)
    assert d.get_param("Rehashes") >= 1 and d.size() == 300
    for q in N.both_radii(viewpoints=[N.ABOVE]) + N.both_radii(min_frames=2):
        assert (~N.no_normal(same_normals(d, h, eig, **q))).sum() > 20
    d.close()
    small = M.distinct_voxels(30, seed=8)
    for stress in (0, 1):
        d, h = pair(L, gpu_ctx, M.LEAF, [("insert", small, 0)], InitialCapacity=64, ProbeStress=stress)
        assert d.get_param("Capacity") == 64
        for q in N.both_radii(min_neighbors=3):
            assert (~N.no_normal(same_normals(d, h, eig, **q))).sum() > 5
        d.close()


# ---- the table after what changes it ------------------------------------------------------------------------------------------
def test_after_growth_reprojection_carving_pruning_and_a_clear(L, gpu_ctx, eig):
    calls = M.growth_calls()
    d, h = pair(L, gpu_ctx, M.LEAF, [("insert", pts, f) for pts, f in calls[:4]], InitialCapacity=64, **N.CARVE_PARAMS)
    assert d.get_param("Rehashes") >= 3
    views = np.array([[0.0, 0.0, 30.0], [40.0, 0.0, 0.0], [0.0, -40.0, 0.0], [3.0, 3.0, -30.0]], np.float32)
    q = dict(radius_leaves=2, viewpoints=views)
    before = same_normals(d, h, eig, **q)
    same_normals(d, h, eig, radius_leaves=1, min_frames=2)
    # a re-projection: the ordinals move apart, voxels merge, sources decide the orientation
    D = np.stack([np.eye(4)] * 4)
    D[1, 0, 3], D[2, 1, 3], D[3, 2, 3] = 0.5, -0.5, 1.0
    assert d.reproject(D) == h.reproject(D.reshape(-1, 16))
    moved = same_normals(d, h, eig, **q)
    assert moved.tobytes() != before.tobytes()
    # carve + prune
    rays = K.ray_cloud(400, seed=3, reach=5.0)
    for m in (d, h):
        N.play(m, [("carve", rays, K.SENSOR, 7), ("carve", rays[::-1], K.SENSOR, 8)])
    assert h.misses().sum() > 50
    for r in (1, 2):
        same_normals(d, h, eig, radius_leaves=r, max_miss_ratio=0.5, viewpoints=views, first_frame=1)
    assert d.prune(1, 0.5) == h.prune(1, 0.5) > 0
    same_normals(d, h, eig, **q)
    # clear + reinsertion
    d.clear(), h.clear()
    assert len(d.normals()) == len(h.normals(eig=eig)) == 0
    for m in (d, h):
        N.play(m, [("insert", calls[4][0], 0)])
    assert len(same_normals(d, h, eig, **q)) == h.size() > 5000
    d.close()


def test_repeated_calls_and_the_capacity_rule(L, gpu_ctx, eig):
    leaf, steps, _, params = N.counted(65)
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    q = dict(radius_leaves=2, min_frames=2, viewpoints=[N.ABOVE])
    first = same_normals(d, h, eig, **q)
    K.same_state(d, h), K.same_state(d, h, 2)
    assert d.normals(**q).tobytes() == first.tobytes() == d.normals(**q).tobytes() and d.get_param("NormalsSeconds") > 0
    K.same_state(d, h), K.same_state(d, h, 2)
    # as lsa_dense_map_get_filtered: the count whatever the capacity, and nothing written past it
    vp = np.array([N.ABOVE], np.float32)
    out = np.zeros(7, L.dense_normal_dtype)
    out["neighbors"][5:] = 0xABCDEF
    call = lambda o, cap: d.L.lsa_dense_map_get_normals(d.h, 2, -1.0, 2, 5, L.ptr(vp), 1, 0, L.ptr(o) if o is not None else None, cap)  # noqa: E731
    assert call(out, 5) == 65 and out[:5].tobytes() == first[:5].tobytes() and (out["neighbors"][5:] == 0xABCDEF).all()
    assert call(None, 0) == 65 and call(out, -1) == L.E_ARG
    d.close()


def test_refusals_leave_the_state(L, gpu_ctx, eig):
    leaf, steps, _, params = N.CASES["seen_through"]()
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    for bad in (dict(radius_leaves=0), dict(radius_leaves=3), dict(min_neighbors=2), dict(radius_leaves=1, min_neighbors=28), dict(min_neighbors=126),
                dict(min_frames=0)):
        with pytest.raises(L.LsaError) as e:
            d.normals(**bad)
        assert e.value.code == L.E_ARG
        with pytest.raises(ValueError):
            h.normals(eig=eig, **bad)
    for bad in ([0.0, 0.0, 1.0], np.zeros((2, 4), np.float32)):
        with pytest.raises(ValueError):
            d.normals(viewpoints=bad)
    assert d.L.lsa_dense_map_get_normals(d.h, 1, -1.0, 2, 5, None, 2, 0, None, 0) == L.E_ARG  # viewpoints promised, none given
    assert d.L.lsa_dense_map_get_normals(d.h, 1, -1.0, 2, 5, None, -1, 0, None, 0) == L.E_ARG
    K.same_state(d, h), K.same_state(d, h, 1, 1.0)
    same_normals(d, h, eig, radius_leaves=1, min_neighbors=27), same_normals(d, h, eig, min_neighbors=125)
    d.close()


# ---- the pipeline --------------------------------------------------------------------------------------------------------------
CARVE = dict(DenseMapCarve=1, DenseMapCarveRange=12.0, DenseMapCarveStride=3)


@pytest.fixture(scope="module")
def drive(L):
    return [L.synth_frame(16, 1000, f) for f in range(6)]


def pipeline_same(L, s, eig):
    """dense_map_normals is the host statement of what the pipeline hands out; returns (viewpoints, first_frame)"""
    views, first = L.dense_map_viewpoints(s)
    assert views.dtype == np.float32 and views.shape == (int(s.get_param("DenseMapFrames")), 3) and first == 0
    pts, vox = L.dense_map_filtered(s, 1, -1.0)
    sources = L.dense_map_sources(s, 1)
    assert len(sources) == len(vox) > 0
    for r in (1, 2):
        for ratio in (-1.0, 1.0):
            fp, fv = L.dense_map_filtered(s, 1, ratio)
            fs = sources[np.isin(vox["key"], fv["key"])]
            for orient in (True, False):
                want = L.dense_normals(fp, fv["key"], fs, r, 5, views if orient else None, first, eig)
                got = L.dense_map_normals(s, 1, ratio, r, 5, orient)
                assert got.tobytes() == want.tobytes(), (r, ratio, orient)
        assert (~N.no_normal(got)).sum() > 0.5 * len(got)
    return views, first


def test_the_pipelines_normals_are_the_host_statement_of_its_map(L, drive, eig):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, DenseMapOnTrajectory=1, LoggingTimeout=-1, **CARVE)
    for f, (pts, stamp) in enumerate(drive):
        s.add_frame(pts, stamp, f)
    views, _ = pipeline_same(L, s, eig)
    P, t, _ = s.trajectory()
    assert len(P) == 6 and views.tobytes() == P[:, :3, 3].astype(np.float32).tobytes()  # the translations of the poses the insertions used
    assert len(L.dense_map_filtered(s, 1, 1.0)[1]) < L.dense_map_size(s)  # the filter leaves something out
    with pytest.raises(L.LsaError) as e:
        L.dense_map_normals(s, radius_leaves=3)
    assert e.value.code == L.E_ARG
    # an applied bent trajectory moves the map and the viewpoints alike
    P2 = P.copy().reshape(-1, 4, 4)
    for i in range(len(P2)):
        a = 0.002 * i
        bend = np.eye(4)
        bend[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        bend[0, 3] = 0.01 * i
        P2[i] = bend @ P2[i]
    s.set_trajectory(P2, t)
    assert s.get_param("DenseMapReprojections") == 1 and s.get_param("DenseMapClears") == 0
    D = L.pose_corrections(P, P2).reshape(-1, 4, 4)
    x, y, z = (views[:, a].astype(np.float64) for a in range(3))
    moved = np.stack([(((D[:, a, 0] * x + D[:, a, 1] * y) + D[:, a, 2] * z) + D[:, a, 3]).astype(np.float32) for a in range(3)], axis=1)
    after, _ = pipeline_same(L, s, eig)
    assert after.tobytes() == moved.tobytes() != views.tobytes()
    L.clear_dense_map(s)
    assert L.dense_map_viewpoints(s)[0].shape == (0, 3) and len(L.dense_map_normals(s)) == 0
    s.close()


def test_without_reprojection_an_applied_trajectory_clears_the_viewpoints_and_off_the_calls_refuse(L, drive):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, LoggingTimeout=-1)
    for f, (pts, stamp) in enumerate(drive[:3]):
        s.add_frame(pts, stamp, f)
    assert L.dense_map_viewpoints(s)[0].shape == (3, 3)
    P, t, _ = s.trajectory()
    P[:, 0, 3] += 0.01 * np.arange(len(P))
    s.set_trajectory(P, t)
    assert s.get_param("DenseMapClears") == 1 and L.dense_map_viewpoints(s)[0].shape == (0, 3)
    s.add_frame(*drive[3], 3)
    assert L.dense_map_viewpoints(s)[0].shape == (1, 3) and L.dense_map_viewpoints(s)[1] == 0
    s.close()
    s = L.Slam(0, EgoMotion=3)
    s.add_frame(*drive[0], 0)
    for call in (lambda: L.dense_map_normals(s), lambda: L.dense_map_viewpoints(s), lambda: L.save_dense_map_pcd_normals(s, "no.pcd")):
        with pytest.raises(L.LsaError) as e:
            call()
        assert e.value.code == L.E_STATE
    assert not os.path.exists("no.pcd")
    s.close()


def test_the_viewpoint_is_the_sensors_not_the_bases(L, drive, eig):
    """one device whose BASE <- LIDAR offset is not the identity: the viewpoint is the translation of Tworld * offset, by the
    library's own product ((a0 * b0 + a1 * b1) + a2 * b2) + a3"""
    a = np.deg2rad(20.0)
    offset = np.eye(4)
    offset[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    offset[:3, 3] = [0.7, -0.3, 1.1]
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, LoggingTimeout=-1)
    s.set_base_to_lidar_offset(offset, device_id=0)
    for f, (pts, stamp) in enumerate(drive[:3]):
        s.add_frame(pts, stamp, f)
    views, _ = pipeline_same(L, s, eig)
    P, _, _ = s.trajectory()
    o = offset[:3, 3]
    want = np.stack([((P[:, r, 0] * o[0] + P[:, r, 1] * o[1]) + P[:, r, 2] * o[2]) + P[:, r, 3] for r in range(3)], axis=1).astype(np.float32)
    assert views.tobytes() == want.tobytes() and np.abs(views - P[:, :3, 3].astype(np.float32)).max() > 0.5
    s.close()


def test_a_call_of_two_devices_keeps_one_viewpoint(L, eig):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, LoggingTimeout=-1)
    for f in range(3):
        frames, stamps, offset = two_device_rig(L, f)
        if f == 0:
            s.set_base_to_lidar_offset(offset, device_id=1)
            s.set_extractor_param(1, "EdgeIntensityGapThreshold", 40.0)
        s.add_frames(frames, stamps, f)
    views, _ = pipeline_same(L, s, eig)
    P, _, _ = s.trajectory()  # device 0, the first frame of every call, is the base
    assert views.shape == (3, 3) and views.tobytes() == P[:, :3, 3].astype(np.float32).tobytes()
    s.close()


# ---- files -----------------------------------------------------------------------------------------------------------------------
PLAIN_HEADER = (b"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z time intensity laser_id device_id label\nSIZE 4 4 4 8 4 2 1 1\n"
                b"TYPE F F F F F U U U\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n")


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_files_with_normals_read_back_and_plain_files_are_what_they_were(L, gpu_ctx, eig, tmp_path, fmt):
    leaf, steps, _, params = N.CASES["oriented"]()
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    q = dict(radius_leaves=1, viewpoints=[N.ABOVE, N.BELOW], first_frame=1)
    want = same_normals(d, h, eig, **q)
    nan = N.no_normal(want)
    assert 0 < nan.sum() < len(want)  # rows without a normal among them
    path = str(tmp_path / f"normals{fmt}.pcd")
    assert d.save_pcd_normals(path, fmt, **q) == len(want) == 81
    assert L.read_pcd_normals(path).view(np.uint32).tobytes() == N.float_bits(want).tobytes()
    assert L.read_pcd(path).tobytes() == d.get()[0].tobytes() and L.pcd_info(path) == (81, fmt)
    head = open(path, "rb").read(400)
    assert b"FIELDS x y z time intensity laser_id device_id label normal_x normal_y normal_z curvature\nSIZE 4 4 4 8 4 2 1 1 4 4 4 4\n" in head
    if fmt == 0:
        assert b" nan nan nan nan\n" in open(path, "rb").read()
    # a dense PCD without normals: the reader refuses and names the file; the file is the writer's of before, byte for byte
    plain = str(tmp_path / f"plain{fmt}.pcd")
    assert d.save_pcd(plain, fmt) == 81
    with pytest.raises(L.LsaError) as e:
        L.read_pcd_normals(plain)
    assert plain in str(e.value)
    written = str(tmp_path / f"written{fmt}.pcd")
    L.write_pcd(written, d.get()[0], fmt)
    data = open(plain, "rb").read()
    assert data == open(written, "rb").read() and data.startswith(PLAIN_HEADER % (81, 81, L.PCD_FORMAT_NAMES[fmt].encode()))
    if fmt == 1:
        assert len(data) == len(PLAIN_HEADER % (81, 81, b"binary")) + 81 * 28
        assert os.path.getsize(path) == head.index(b"DATA binary\n") + len(b"DATA binary\n") + 81 * 44
    with pytest.raises(L.LsaError):
        d.save_pcd_normals(str(tmp_path / "bad.pcd"), fmt, radius_leaves=3)
    assert not os.path.exists(str(tmp_path / "bad.pcd"))
    d.close()


def test_the_pipelines_file_is_its_map_and_its_normals(L, drive, tmp_path):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, **CARVE)
    for f, (pts, stamp) in enumerate(drive[:4]):
        s.add_frame(pts, stamp, f)
    path = str(tmp_path / "dense_normals.pcd")
    pts, _ = L.dense_map_filtered(s, 1, 1.0)
    normals = L.dense_map_normals(s, 1, 1.0, 2, 5, True)
    assert L.save_dense_map_pcd_normals(s, path, L.PCD_BINARY, 1, 1.0, 2, 5, True) == len(pts) == len(normals) > 5000
    assert L.read_pcd(path).tobytes() == pts.tobytes() and L.read_pcd_normals(path).view(np.uint32).tobytes() == N.float_bits(normals).tobytes()
    unoriented = L.dense_map_normals(s, 1, 1.0, 2, 5, False)
    assert unoriented.tobytes() != normals.tobytes() and (unoriented["neighbors"] == normals["neighbors"]).all()
    s.close()
