"""Free-space carving of the dense map on the device (lidarslam_amd/csrc/lsa_dense_carve.hip: k_dense_carve, the filtered
exports, lsa_dense_map_prune) against DenseMapHost, byte for byte on points, voxel records, sources and misses, and on the
count of rays: the walk's cases, wavefront edges, the scene, long probe sequences, growth, re-projection, the fused frame
path, the pipeline, files, refusals.  Cases: tests/dense_carve_cases.py."""
import os

import numpy as np
import pytest

import dense_carve_cases as K
import dense_map_cases as M
from conftest import two_device_rig
from test_gpu_dense_map import NFRAMES, PIPE_LEAF, frame_path, transform_frame_at

pytestmark = pytest.mark.gpu


def same(device, host):
    n = K.same_state(device, host)
    assert device.get_param("Rays") == host.rays
    return n


class Pair:
    """a device map and the host statement, fed alike"""

    def __init__(self, L, ctx, leaf=K.LEAF, margin_leaves=2.0, max_range=30.0, stride=1, **params):
        self.d = L.DenseMap(ctx, leaf, CarveMarginLeaves=margin_leaves, CarveRange=max_range, CarveStride=stride, **params)
        self.h = L.DenseMapHost(leaf)
        self.kw = dict(margin_leaves=margin_leaves, max_range=max_range, stride=stride)

    def insert(self, pts, frame):
        self.d.insert_points(pts, frame)
        self.h.insert(pts, frame)

    def carve(self, pts, origins, frame):
        self.d.carve_points(pts, origins, frame)
        self.h.carve(pts, origins, frame, **self.kw)

    def same(self):
        return same(self.d, self.h)

    def close(self):
        self.d.close()


# ---- 1. the walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.RAY_CASES))
def test_every_ray_case_as_one_call(L, gpu_ctx, name):
    pts, org, kw = K.ray(name)
    p = Pair(L, gpu_ctx, **kw)
    p.insert(K.ray_scene(name), 0)
    p.carve(pts, org, 1)
    visited = K.walk(name)
    assert p.same() == p.h.size() > 0 and p.h.rays == (visited is not None)
    assert int(p.h.misses().sum()) == (len(visited) if visited else 0)  # the map holds every voxel of the walk and its surroundings
    p.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_wavefront_edges(L, gpu_ctx, n):
    pts = K.ray_cloud(n, seed=n)
    org = np.random.default_rng(n).uniform(-1, 1, (n, 3)).astype(np.float32)
    p = Pair(L, gpu_ctx)
    p.insert(K.ray_cloud(4097, seed=7), 0)
    p.carve(pts, org, 1)
    p.carve(pts, org[:1], 2)  # one origin for all
    assert p.same() > 3000 and (n < 63 or p.h.misses().sum() > 0)
    p.close()


def test_one_wavefront_of_no_steps_and_longest_rays(L, gpu_ctx):
    pts, org, leaf, max_range = K.mixed_wavefront()
    p = Pair(L, gpu_ctx, leaf=leaf, margin_leaves=0.0, max_range=max_range)
    lengths = [len(w) for w in K.walks(pts, org, leaf, margin_leaves=0.0, max_range=max_range)]
    assert lengths[::2] == [1] * 32 and min(lengths[1::2]) > 4096
    # a map of voxels along the long rays, every 5th of each
    along = np.concatenate([np.asarray(w[::5]) for w in K.walks(pts, org, leaf, margin_leaves=0.0, max_range=max_range)[1::2]])
    p.insert(K.voxel_points(np.unique(along, axis=0), leaf=leaf), 0)
    p.carve(pts, org, 1)
    assert p.same() > 1000 and p.h.rays == 64 and p.h.misses().sum() > 1000
    p.close()


# ---- 2. the scene: filter, prune, and the table afterwards --------------------------------------------------------------------
def test_the_scene_filtered_pruned_and_inserted_into_again(L, gpu_ctx):
    h, wall, obj = K.host_scene()
    d, _, _ = K.carved_scene(lambda: L.DenseMap(gpu_ctx, K.LEAF))
    assert same(d, h) == len(wall) + len(obj)
    for ratio in K.RATIOS:
        for m in (1, 2, 8):
            K.same_state(d, h, m, ratio)
    assert len(d.get(1, 1.0)[1]) == len(wall) and d.get_param("Capacity") == 1 << 16
    bytes_before = d.bytes()
    assert d.prune(1, 1.0) == h.prune(1, 1.0) == len(obj) == d.get_param("Pruned")
    assert same(d, h) == d.size() == len(wall) and d.get_param("Prunes") == 1
    assert d.get_param("Capacity") == 512 and d.bytes() < bytes_before  # the smallest power of two with capacity / 2 >= 169
    assert d.prune(1, 1.0) == 0 and d.get_param("Capacity") == 512
    # the table still works: old voxels are found, new ones claimed, the next carve counts
    calls, _, _ = K.scene()
    for m in (d, h):
        (m.insert_points if m is d else m.insert)(calls[0][0], 8)
    d.carve_points(calls[7][0], K.SENSOR, 9)
    h.carve(calls[7][0], K.SENSOR, 9)
    assert same(d, h) == len(wall) + 8 and d.skipped() == 0
    d.close()


def test_probe_stress_gives_the_same_misses(L, gpu_ctx):
    pts = K.ray_cloud(700, seed=3)
    rays = K.ray_cloud(300, seed=4, reach=9.0)  # most end in voxels the map does not hold: absent keys along long sequences
    org = np.zeros((1, 3), np.float32)
    stressed, plain = Pair(L, gpu_ctx, InitialCapacity=64, ProbeStress=1), Pair(L, gpu_ctx)
    for p in (stressed, plain):
        p.insert(pts[:400], 0)
        p.carve(rays, org, 1)
        p.insert(pts[400:], 2)
        p.carve(rays[::-1], org, 3)
        p.same()
    assert stressed.d.get_param("Rehashes") >= 1 and stressed.h.misses().sum() > 200
    assert stressed.d.misses().tobytes() == plain.d.misses().tobytes()
    stressed.close(), plain.close()


def test_misses_survive_growth(L, gpu_ctx):
    calls = M.growth_calls()
    org = np.array([[0.3, -0.2, 0.1]], np.float32)
    small, large = Pair(L, gpu_ctx, InitialCapacity=64), Pair(L, gpu_ctx, InitialCapacity=1 << 17)
    for p in (small, large):
        for pts, frame in calls[:3]:
            p.insert(pts, 2 * frame)
        p.carve(calls[4][0][::3], org, 5)
        before = p.d.get_param("Rehashes")
        for pts, frame in calls[3:]:
            p.insert(pts, 2 * frame)  # (the small table doubles under these, carrying the misses)
        assert (p.d.get_param("Rehashes") > before) == (p is small)
        p.carve(calls[2][0][::2], org, 9)
        assert p.same() == M.BATCH and p.h.misses().max() == 2
    assert small.d.misses().tobytes() == large.d.misses().tobytes()
    small.close(), large.close()


def test_reproject_after_carving(L, gpu_ctx):
    h, wall, obj = K.host_scene()
    d, _, _ = K.carved_scene(lambda: L.DenseMap(gpu_ctx, K.LEAF))
    D = np.stack([np.eye(4)] * K.SCENE_FRAMES)
    D[1::2, 1, 3] = 0.5  # the voxels whose points odd ordinals measured move one voxel in y: object voxels meet
    total = int(h.misses().sum())
    assert d.reproject(D) == h.reproject(D.reshape(-1, 16)) == 0
    assert same(d, h) < len(wall) + len(obj) and int(h.misses().sum()) == total
    calls, _, _ = K.scene()
    d.carve_points(calls[7][0], K.SENSOR, 7)  # ordinal 7 has counted already, also in the merged voxels
    h.carve(calls[7][0], K.SENSOR, 7)
    same(d, h)
    d.carve_points(calls[7][0], K.SENSOR, 8)
    h.carve(calls[7][0], K.SENSOR, 8)
    assert same(d, h) > 0 and int(h.misses().sum()) > total
    d.close()


def test_clear_zeroes_everything(L, gpu_ctx):
    d, _, _ = K.carved_scene(lambda: L.DenseMap(gpu_ctx, K.LEAF))
    d.prune(1, 1.0)
    assert d.get_param("Rays") > 0 and d.get_param("Pruned") > 0 and d.misses().sum() == 0
    d.clear()
    assert d.size() == 0 and d.get_param("Rays") == 0 and d.get_param("Pruned") == 0 and len(d.misses()) == 0
    h, _, _ = K.host_scene()  # ordinals start again, and no miss of before comes back
    calls, _, _ = K.scene()
    for pts, f in calls:
        d.insert_points(pts, f)
        d.carve_points(pts, K.SENSOR, f)
    same(d, h)
    d.close()


# ---- 3. the fused path ---------------------------------------------------------------------------------------------------------
FUSED = dict(CarveRange=15.0)


@pytest.mark.parametrize("interpolate", [False, True])
@pytest.mark.parametrize("time_offset", [0.0, 0.0125])
def test_carve_frame_is_carve_points_of_the_transformed_frame_and_its_origins(L, gpu_ctx, interpolate, time_offset):
    leaf = 0.2
    fused, plain, h = L.DenseMap(gpu_ctx, leaf, **FUSED), L.DenseMap(gpu_ctx, leaf, **FUSED), L.DenseMapHost(leaf)
    for f in range(2):
        pts, _ = L.synth_frame(16, 1000, f)
        gpu_ctx.upload_frame(pts)
        H0, H1 = L.synth_pose(f), (L.synth_pose(f + 1) if interpolate else None)
        world = transform_frame_at(L, gpu_ctx, H0, H1, -0.1, 0.0, time_offset)
        origins = L.frame_origins_at(gpu_ctx, H0, H1, -0.1, 0.0, time_offset)
        assert origins.shape == (world.size, 3) and origins.dtype == np.float32
        if interpolate:
            assert len(np.unique(origins, axis=0)) > 100  # the sensor moves within the frame
        else:
            assert (origins == np.asarray(H0, np.float64)[:3, 3].astype(np.float32)).all()
        fused.insert_frame(f, H0, H1, -0.1, 0.0, time_offset)
        fused.carve_frame(f, H0, H1, -0.1, 0.0, time_offset)
        plain.insert_points(world, f)
        plain.carve_points(world, origins, f)
        h.insert(world, f)
        h.carve(world, origins, f, max_range=15.0)
    assert h.skipped == 0 and h.size() > 5000 and h.misses().sum() > 100
    same(fused, h)
    same(plain, h)
    K.same_state(fused, h, 1, 1.0)
    fused.close(), plain.close()


def test_a_frame_uploaded_in_wire_format_waits_for_the_carve_that_reads_its_buffer(L):
    """the case of tests/test_gpu_dense_map.py with carving on: the carve reads the frame's buffer after the insertion has,
    so the next upload must wait for it, not for the insertion"""
    from test_gpu_pipeline import VELODYNE_LAYOUT, wire_records

    leaf = 0.2
    ctx = L.Context(0)
    fused, h = L.DenseMap(ctx, leaf, **FUSED), L.DenseMapHost(leaf)
    worlds = []
    for f in range(4):
        pts, _ = L.synth_frame(16, 1000, f)
        ctx.upload_wire_frame(wire_records(pts), VELODYNE_LAYOUT)
        H0, H1 = L.synth_pose(f), L.synth_pose(f + 1)
        worlds.append((transform_frame_at(L, ctx, H0, H1, -0.1, 0.0, 0.0), L.frame_origins_at(ctx, H0, H1, -0.1, 0.0)))
        fused.insert_frame(f, H0, H1, -0.1, 0.0)
        fused.carve_frame(f, H0, H1, -0.1, 0.0)  # nothing waits for it before the next upload
    for f, (world, origins) in enumerate(worlds):
        h.insert(world, f)
        h.carve(world, origins, f, max_range=15.0)
    assert h.skipped == 0 and h.size() > 8000 and h.misses().sum() > 100
    same(fused, h)
    fused.close()
    ctx.close()


# ---- 4. the pipeline -----------------------------------------------------------------------------------------------------------
CARVE = dict(DenseMapCarveRange=12.0, DenseMapCarveStride=3)  # (what keeps the host statement of 12 frames quick)


@pytest.fixture(scope="module")
def drive(L):
    return [L.synth_frame(16, 1000, f) for f in range(NFRAMES)]


@pytest.fixture(scope="module")
def without(L, drive):
    s = L.Slam(0, EgoMotion=3)
    for f, (pts, stamp) in enumerate(drive):
        s.add_frame(pts, stamp, f)
    out = frame_path(L, s)
    for call in (lambda: L.dense_map_filtered(s, 1, 1.0), lambda: L.dense_map_misses(s), lambda: L.prune_dense_map(s), lambda: L.save_dense_map_pcd_filtered(s, "no.pcd")):
        with pytest.raises(L.LsaError) as e:
            call()  # off: the calls refuse
        assert e.value.code == L.E_STATE
    assert s.get_param("DenseMapCarve") == 0 and s.get_param("DenseMapRays") == 0 and not os.path.exists("no.pcd")
    s.close()
    return out


class PipelineMap:
    """the pipeline's map with the methods same_state asks for"""

    def __init__(self, L, s):
        self.L, self.s = L, s

    def get(self, m=1, r=-1.0):
        return self.L.dense_map_filtered(self.s, m, r)

    def misses(self, m=1, r=-1.0):
        return self.L.dense_map_misses(self.s, m, r)

    def sources(self, m=1, r=-1.0):
        assert r < 0
        return self.L.dense_map_sources(self.s, m)


def pipeline_same(L, s, h):
    n = K.same_state(PipelineMap(L, s), h)
    pm = PipelineMap(L, s)
    for ratio in (0.0, 1.0):
        assert pm.get(1, ratio)[1].tobytes() == h.get(1, ratio)[1].tobytes() and pm.misses(1, ratio).tobytes() == h.misses(1, ratio).tobytes()
    assert s.get_param("DenseMapRays") == h.rays
    return n


@pytest.mark.parametrize("mode,hint", [(1, True), (1, False), (2, False)])
def test_the_pipelines_carved_map_is_the_host_statement_of_its_registered_frames(L, drive, without, mode, hint):
    s = L.Slam(0, EgoMotion=3, DenseMap=mode, DenseMapLeafSize=PIPE_LEAF, DenseMapCarve=1, **CARVE)
    h = L.DenseMapHost(PIPE_LEAF)
    ordinal, kf = 0, 0
    for f, (pts, stamp) in enumerate(drive):
        if hint and f + 1 < len(drive):
            s.hint_next_frame(drive[f + 1][0])
        s.add_frame(pts, stamp, f)
        now = int(s.stats()[13])
        if mode == 1 or now != kf:
            world, origins = s.registered_frame().copy(), L.registered_frame_origins(s)
            assert origins.shape == (world.size, 3)
            h.insert(world, ordinal)
            h.carve(world, origins, ordinal, max_range=12.0, stride=3)
            ordinal += 1
        kf = now
    assert h.skipped == 0 and 1 < ordinal <= NFRAMES and h.rays > 1000 * ordinal and h.misses().sum() > 100
    assert pipeline_same(L, s, h) == L.dense_map_size(s) > 5000
    assert frame_path(L, s) == without  # the frame path does not notice
    if hint:
        assert s.get_param("UploadsAdopted") >= NFRAMES - 2
    s.close()


def test_a_call_of_two_devices_inserts_both_frames_before_it_carves_either(L):
    """leaf 1.0: at the finer leaves of the other tests no voxel of this rig is hit by the second device alone and crossed by
    a ray of the first, and the two orders give the same misses"""
    leaf = 1.0
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=leaf, DenseMapCarve=1)
    h, one_by_one = L.DenseMapHost(leaf), L.DenseMapHost(leaf)
    for f in range(3):
        frames, stamps, offset = two_device_rig(L, f)
        if f == 0:
            s.set_base_to_lidar_offset(offset, device_id=1)
            s.set_extractor_param(1, "EdgeIntensityGapThreshold", 40.0)
        s.add_frames(frames, stamps, f)
        world, origins = s.registered_frame().copy(), L.registered_frame_origins(s)
        n0 = frames[0].size
        assert world.size == n0 + frames[1].size == len(origins)
        h.insert(world[:n0], f)
        h.insert(world[n0:], f)
        h.carve(world[:n0], origins[:n0], f)
        h.carve(world[n0:], origins[n0:], f)
        for part in (slice(0, n0), slice(n0, None)):  # what must NOT happen: the first device carved before the second is in
            one_by_one.insert(world[part], f)
            one_by_one.carve(world[part], origins[part], f)
    assert (h.misses() != one_by_one.misses()).sum() > 20, "the rig does not tell the two orders apart"
    pipeline_same(L, s, h)
    s.close()


def test_a_pruned_pipeline_map_saves_and_reads_back_as_the_filtered_map(L, drive, tmp_path):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, DenseMapCarve=1, DenseMapOnTrajectory=1, **CARVE)
    for f, (pts, stamp) in enumerate(drive[:5]):
        s.add_frame(pts, stamp, f)
    everything, (seen, _) = L.dense_map_size(s), L.dense_map_filtered(s, 1, 1.0)
    path = str(tmp_path / "seen.pcd")
    assert L.save_dense_map_pcd_filtered(s, path, 1, 1, 1.0) == seen.size and L.read_pcd(path).tobytes() == seen.tobytes()
    assert L.prune_dense_map(s, 1, 1.0) == everything - seen.size == s.get_param("DenseMapPruned")
    assert L.dense_map(s)[0].tobytes() == seen.tobytes() and L.dense_map_size(s) == seen.size
    path = str(tmp_path / "pruned.pcd")
    assert L.save_dense_map_pcd(s, path, 1, 1) == seen.size and L.read_pcd(path).tobytes() == seen.tobytes()
    s.add_frame(*drive[5], 5)  # mapping goes on in the pruned table
    assert L.dense_map_size(s) > seen.size
    L.clear_dense_map(s)
    assert L.dense_map_size(s) == 0 and s.get_param("DenseMapRays") == 0 and s.get_param("DenseMapPruned") == 0
    s.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(L, gpu_ctx):
    d = L.DenseMap(gpu_ctx, 0.01)
    for bad in (4096 * 0.01 * 1.001, 0.0, -1.0, float("nan")):
        with pytest.raises(L.LsaError) as e:
            d.set("CarveRange", bad)
        assert e.value.code == L.E_ARG
    d.set("CarveRange", 40.0)  # 4000 leaves
    assert d.get_param("CarveRange") == 40.0 and d.get_param("CarveMarginLeaves") == 2 and d.get_param("CarveStride") == 1
    for name, bad in (("CarveStride", 0), ("CarveStride", 1.5), ("CarveMarginLeaves", -1)):
        with pytest.raises(L.LsaError) as e:
            d.set(name, bad)
        assert e.value.code == L.E_ARG
    d.close()
    d = L.DenseMap(gpu_ctx, K.LEAF)
    pts, org = K.ray_cloud(10), np.zeros((1, 3), np.float32)
    d.insert_points(pts, 5)
    d.carve_points(pts, org, 6)
    for call in (lambda: d.carve_points(pts, org, 5), lambda: d.insert_points(pts, 5), lambda: d.carve_points(pts, org, -(1 << 31)),
                 lambda: d.carve_points(pts, np.zeros((2, 3), np.float32), 7)):
        with pytest.raises(L.LsaError) as e:
            call()  # decreasing ordinals, the ordinal kept for "none", neither one origin nor one per point
        assert e.value.code == L.E_ARG
    h = L.DenseMapHost(K.LEAF)
    h.insert(pts, 5)
    h.carve(pts, org, 6)
    same(d, h)
    d.close()
