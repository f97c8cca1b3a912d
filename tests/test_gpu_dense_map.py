"""The dense point-cloud map on the device (lidarslam_amd/csrc/lsa_dense_map.hip) against DenseMapHost, byte for byte on points
and voxel records: the table alone, growth, long probe sequences, refusal, the fused frame path, the pipeline, what clears
the map, files.  Cases: tests/dense_map_cases.py."""
import os

import numpy as np
import pytest

import dense_map_cases as K
from conftest import two_device_rig

pytestmark = pytest.mark.gpu


def same(device, host, min_frames=1):
    dp, dv = device.get(min_frames) if hasattr(device, "get") else device
    hp, hv = host.get(min_frames)
    assert dv.tobytes() == hv.tobytes(), (len(dv), len(hv))
    assert dp.tobytes() == hp.tobytes()
    return len(hv)


def device_map(L, ctx, calls, leaf=K.LEAF, **params):
    d = L.DenseMap(ctx, leaf, **params)
    for pts, frame in calls:
        d.insert_points(pts, frame)
    return d


# ---- 1. the table alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.SIZES)
def test_distinct_voxels(L, gpu_ctx, n):
    calls = [(K.distinct_voxels(n), 0)]
    h = K.assert_nothing_skipped(L.DenseMapHost, calls)
    d = device_map(L, gpu_ctx, calls)
    assert same(d, h) == n == d.size() and d.skipped() == 0
    d.close()


def test_one_voxel_holds_a_whole_call(L, gpu_ctx):
    calls = [(K.one_voxel(4097), 0), (K.one_voxel(4097), 1)]
    h = K.assert_nothing_skipped(L.DenseMapHost, calls)
    d = device_map(L, gpu_ctx, calls)
    assert same(d, h) == 1
    pts, vox = d.get()
    assert vox["count"][0] == 2 * 4097 and vox["frames"][0] == 2 and pts[0].tobytes() == calls[0][0][0].tobytes()
    d.close()


@pytest.mark.parametrize("order", ["contiguous", "interleaved", "reversed"])
def test_runs_in_three_arrival_orders(L, gpu_ctx, order):
    first = K.runs(order)
    second = K.runs("interleaved")[::2].copy()  # a second call onto half of every long run
    second["intensity"] += np.float32(1)
    calls = [(first, 0), (second, 1)]
    h = K.assert_nothing_skipped(L.DenseMapHost, calls)
    d = device_map(L, gpu_ctx, calls)
    same(d, h)
    same(d, h, 2)
    d.close()


@pytest.mark.parametrize("name", sorted(K.PROPERTY_CASES))
def test_the_properties_of_the_definition(L, gpu_ctx, name):
    calls = K.PROPERTY_CASES[name]()
    h = K.host_map(L.DenseMapHost, calls)
    assert (h.skipped == 0) == (name != "skipping")
    d = device_map(L, gpu_ctx, calls)
    assert same(d, h) == h.size() and d.skipped() == h.skipped
    for m in (2, 3, 9):
        same(d, h, m)
    with pytest.raises(L.LsaError) as e:
        d.insert_points(calls[0][0], calls[-1][1] - 1)  # ordinals must not decrease
    assert e.value.code == L.E_ARG
    same(d, h)
    d.clear()
    assert d.size() == 0 and d.skipped() == 0 and len(d.get()[1]) == 0
    d.close()


# ---- 2. growth ---------------------------------------------------------------------------------------------------------------
def test_growth_gives_the_map_of_a_table_that_started_large(L, gpu_ctx):
    calls = K.growth_calls()
    h = K.assert_nothing_skipped(L.DenseMapHost, calls)
    small = L.DenseMap(gpu_ctx, K.LEAF, InitialCapacity=64)
    large = L.DenseMap(gpu_ctx, K.LEAF, InitialCapacity=1 << 17)
    rehashes = []
    for pts, frame in calls:
        small.insert_points(pts, frame)
        large.insert_points(pts, frame)
        rehashes.append(small.get_param("Rehashes"))
    assert rehashes[0] == 0 and rehashes[-1] >= 3 and rehashes[2] > rehashes[1] and rehashes[4] > rehashes[3]  # doublings before the calls that revisit
    assert large.get_param("Rehashes") == 0 and large.get_param("Capacity") == 1 << 17
    assert same(small, h) == K.BATCH
    same(large, h)
    assert small.get_param("Capacity") >= 2 * K.BATCH and small.bytes() >= 64 * small.get_param("Capacity")
    small.close(), large.close()


# ---- 3. long probe sequences -------------------------------------------------------------------------------------------------
def test_probe_stress_changes_nothing(L, gpu_ctx):
    calls = K.stress_calls()
    h = K.assert_nothing_skipped(L.DenseMapHost, calls)
    d = L.DenseMap(gpu_ctx, K.LEAF, InitialCapacity=64, ProbeStress=1)
    for pts, frame in calls:
        d.insert_points(pts, frame)
    assert same(d, h) == 2048 and d.get_param("Rehashes") >= 1
    with pytest.raises(L.LsaError) as e:
        d.set("ProbeStress", 0)  # the keys in the table were placed under the other rule
    assert e.value.code == L.E_STATE
    d.close()


# ---- 4. refusal --------------------------------------------------------------------------------------------------------------
def test_an_insertion_over_the_cap_is_refused_whole(L, gpu_ctx):
    a, b = K.distinct_voxels(1000, seed=1), K.distinct_voxels(4097, seed=2)
    d = L.DenseMap(gpu_ctx, K.LEAF, InitialCapacity=4096)
    d.insert_points(a, 0)
    cap = int(d.get_param("Capacity"))
    assert cap == 4096
    d.set("MaxBytes", 64 * cap)  # the table as it is, and not a slot more
    before = d.get()
    with pytest.raises(L.LsaError) as e:
        d.insert_points(b, 1)
    assert e.value.code == L.E_CAPACITY and "MaxBytes" in str(e.value)
    after = d.get()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and d.get_param("Capacity") == cap
    d.set("MaxBytes", 64 * 4 * cap)
    d.insert_points(b, 1)
    h = K.assert_nothing_skipped(L.DenseMapHost, [(a, 0), (b, 1)])
    same(d, h)
    d.close()


# ---- 5. the fused path -------------------------------------------------------------------------------------------------------
def transform_frame_at(L, ctx, H0, H1, t0, t1, time_offset):
    n = ctx.L.lsa_frame_size(ctx.h)
    out = np.zeros(n, L.POINT_DTYPE)
    interp = H1 is not None
    rc = ctx.L.lsa_transform_frame_at(ctx.h, int(interp), L.ptr(L.pose16(H0)), L.ptr(L.pose16(H1)) if interp else None, t0, t1, time_offset, L.ptr(out), n)
    assert rc == n
    return out


@pytest.mark.parametrize("interpolate", [False, True])
@pytest.mark.parametrize("time_offset", [0.0, 0.0125])
def test_insert_frame_is_insert_points_of_the_transformed_frame(L, gpu_ctx, interpolate, time_offset):
    leaf = 0.2
    fused, plain, h = L.DenseMap(gpu_ctx, leaf), L.DenseMap(gpu_ctx, leaf), L.DenseMapHost(leaf)
    for f in range(2):
        pts, _ = L.synth_frame(16, 1000, f)
        gpu_ctx.upload_frame(pts)
        H0, H1 = L.synth_pose(f), (L.synth_pose(f + 1) if interpolate else None)
        world = transform_frame_at(L, gpu_ctx, H0, H1, -0.1, 0.0, time_offset)
        fused.insert_frame(f, H0, H1, -0.1, 0.0, time_offset)
        plain.insert_points(world, f)
        h.insert(world, f)
    assert h.skipped == 0 and h.size() > 5000
    same(fused, h)
    same(plain, h)
    same(fused, h, 2)
    fused.close(), plain.close()


def test_a_frame_uploaded_in_wire_format_waits_for_the_insertion_that_reads_its_buffer(L):
    """the wire-format uploads rewrite the context's own frame buffer on the registration stream while the fused insertion of
    the frame before may still read it on the look-ahead stream: every frame goes in as it was when it was inserted"""
    from test_gpu_pipeline import VELODYNE_LAYOUT, wire_records

    leaf = 0.2
    ctx = L.Context(0)
    fused, h = L.DenseMap(ctx, leaf), L.DenseMapHost(leaf)
    worlds = []
    for f in range(4):  # frame 0 goes through the host (resolution estimate), the others are converted on the device
        pts, _ = L.synth_frame(16, 1000, f)
        ctx.upload_wire_frame(wire_records(pts), VELODYNE_LAYOUT)
        H0, H1 = L.synth_pose(f), L.synth_pose(f + 1)
        worlds.append(transform_frame_at(L, ctx, H0, H1, -0.1, 0.0, 0.0))
        fused.insert_frame(f, H0, H1, -0.1, 0.0)  # nothing waits for it before the next upload
    for f, world in enumerate(worlds):
        h.insert(world, f)
    assert h.skipped == 0 and h.size() > 8000
    same(fused, h)
    fused.close()
    ctx.close()


# ---- 6. the pipeline ---------------------------------------------------------------------------------------------------------
NFRAMES, PIPE_LEAF = 12, 0.2


@pytest.fixture(scope="module")
def drive(L):
    return [L.synth_frame(16, 1000, f) for f in range(NFRAMES)]


def run(L, drive, mode, hint=False, **params):
    """-> (slam, [registered frame or None per frame], [keyframe?])"""
    s = L.Slam(0, EgoMotion=3, **params)
    if mode:
        s.set_param("DenseMap", mode)
        s.set_param("DenseMapLeafSize", PIPE_LEAF)
    registered, keyframe, kf = [], [], 0
    for f, (pts, stamp) in enumerate(drive):
        if hint and f + 1 < len(drive):
            s.hint_next_frame(drive[f + 1][0])
        s.add_frame(pts, stamp, f)
        now = int(s.stats()[13])
        keyframe.append(now != kf)
        kf = now
        registered.append(s.registered_frame().copy() if mode else None)
    return s, registered, keyframe


def frame_path(L, s):
    P, t, cov = s.trajectory()
    return [s.world_transform().tobytes(), s.covariance().tobytes(), P.tobytes(), t.tobytes()] + [s.map(k).tobytes() for k in (L.EDGE, L.PLANE, L.BLOB)]


@pytest.fixture(scope="module")
def without(L, drive):
    s, _, _ = run(L, drive, 0)
    out = frame_path(L, s)
    with pytest.raises(L.LsaError) as e:
        L.dense_map_size(s)  # off: the calls refuse
    assert e.value.code == L.E_STATE
    assert s.get_param("DenseMap") == 0 and s.get_param("DenseMapVoxels") == 0
    s.close()
    return out


@pytest.mark.parametrize("mode,hint", [(1, True), (1, False), (2, False)])
def test_the_pipelines_map_is_the_host_statement_of_its_registered_frames(L, drive, without, mode, hint):
    s, registered, keyframe = run(L, drive, mode, hint)
    h = L.DenseMapHost(PIPE_LEAF)
    ordinal = 0
    for pts, kf in zip(registered, keyframe):
        if mode == 1 or kf:
            h.insert(pts, ordinal)
            ordinal += 1
    assert h.skipped == 0 and ordinal == (NFRAMES if mode == 1 else sum(keyframe)) and 1 < sum(keyframe)
    assert same(L.dense_map(s), h) == L.dense_map_size(s) == s.get_param("DenseMapVoxels") > 5000
    for m in (2, 3):
        assert 0 < same(L.dense_map(s, m), h, m) < h.size()
    assert s.get_param("DenseMapSkipped") == 0 and s.get_param("DenseMapRefusedFrames") == 0 and s.get_param("DenseMapBytes") >= 64 * 2 * h.size()
    assert frame_path(L, s) == without  # the frame path does not notice
    if hint:
        assert s.get_param("UploadsAdopted") >= NFRAMES - 2
    s.close()


def test_a_refused_frame_is_counted_and_the_drive_goes_on(L, drive):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, DenseMapMaxBytes=64 * 1024)
    for f, (pts, stamp) in enumerate(drive[:3]):
        s.add_frame(pts, stamp, f)
    assert s.get_param("DenseMapRefusedFrames") == 3 and L.dense_map_size(s) == 0 and "MaxBytes" in s.L.lsa_slam_last_error(s.h).decode()
    s.set_param("DenseMapMaxBytes", 1 << 30)
    s.add_frame(*drive[3], 3)
    assert s.get_param("DenseMapRefusedFrames") == 3 and L.dense_map_size(s) > 5000
    s.close()


def test_a_call_of_two_devices_is_inserted_whole_or_refused_whole(L):
    """the first device's frame alone would be refused and the second's alone would fit: neither goes in"""
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF)
    assert s.get_param("DenseMapMaxBytes") == 16 * 2.0**30  # the documented default, before any map exists
    frames, stamps, offset = two_device_rig(L, 0)
    frames[1] = frames[1][:500].copy()
    assert frames[0].size > 1024 >= 2 * frames[1].size
    s.set_base_to_lidar_offset(offset, device_id=1)
    s.set_extractor_param(1, "EdgeIntensityGapThreshold", 40.0)
    s.set_param("DenseMapMaxBytes", 64 * 2048)  # 2 048 slots: room for 1 024 points
    s.add_frames(frames, stamps, 0)
    assert s.get_param("DenseMapRefusedFrames") == 1 and s.get_param("DenseMapFrames") == 0 and L.dense_map_size(s) == 0
    s.set_param("DenseMapMaxBytes", 1 << 30)
    frames, stamps, _ = two_device_rig(L, 1)
    s.add_frames(frames, stamps, 1)
    assert s.get_param("DenseMapRefusedFrames") == 1 and s.get_param("DenseMapFrames") == 1 and L.dense_map_size(s) > 1000
    assert s.get_param("DenseMapCapacity") >= 2 * L.dense_map_size(s)
    s.close()


def test_two_devices_of_one_call_count_one_frame(L):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF)
    h = L.DenseMapHost(PIPE_LEAF)
    calls = 4
    for f in range(calls):
        frames, stamps, offset = two_device_rig(L, f)
        if f == 0:
            s.set_base_to_lidar_offset(offset, device_id=1)
            s.set_extractor_param(1, "EdgeIntensityGapThreshold", 40.0)
        s.add_frames(frames, stamps, f)
        world = s.registered_frame().copy()
        assert world.size == frames[0].size + frames[1].size
        h.insert(world[: frames[0].size], f)
        h.insert(world[frames[0].size :], f)
    assert h.skipped == 0
    same(L.dense_map(s), h)
    _, vox = L.dense_map(s)
    assert vox["frames"].max() == calls and set(np.unique(vox["last_frame"])) <= set(range(calls))
    s.close()


# ---- 7. what clears the map ----------------------------------------------------------------------------------------------------
def test_an_applied_trajectory_reset_and_clear_empty_the_map(L, drive):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, LoggingTimeout=-1)
    for f, (pts, stamp) in enumerate(drive[:6]):
        s.add_frame(pts, stamp, f)
    assert L.dense_map_size(s) > 5000 and s.get_param("DenseMapClears") == 0
    P, t, _ = s.trajectory()
    P2 = P.copy().reshape(-1, 4, 4)
    P2[:, 0, 3] += 0.01 * np.arange(P2.shape[0])
    s.set_trajectory(P2, t)
    assert L.dense_map_size(s) == 0 and s.get_param("DenseMapClears") == 1
    # mapping goes on and fills the map again, with ordinals that start again
    h = L.DenseMapHost(PIPE_LEAF)
    for i, f in enumerate(range(6, 9)):
        s.add_frame(*drive[f], f)
        h.insert(s.registered_frame().copy(), i)
    assert same(L.dense_map(s), h) > 5000
    L.clear_dense_map(s)
    assert L.dense_map_size(s) == 0 and s.get_param("DenseMapClears") == 2
    s.add_frame(*drive[9], 9)
    assert L.dense_map_size(s) > 1000
    s.reset()
    assert L.dense_map_size(s) == 0 and s.get_param("DenseMapClears") == 3
    h = L.DenseMapHost(PIPE_LEAF)
    for f in range(2):
        s.add_frame(*drive[f], f)
        h.insert(s.registered_frame().copy(), f)
    same(L.dense_map(s), h)
    s.close()


def test_a_map_switched_off_does_not_come_back_stale(L, drive):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF)
    for f, (pts, stamp) in enumerate(drive[:3]):
        s.add_frame(pts, stamp, f)
    assert L.dense_map_size(s) > 5000
    s.set_param("DenseMap", 0)
    s.add_frame(*drive[3], 3)  # not inserted
    s.reset()  # the poses the map was made under are gone
    s.set_param("DenseMap", 1)
    assert L.dense_map_size(s) == 0 and s.get_param("DenseMapClears") == 1
    s.close()


# ---- 8. files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_a_saved_map_reads_back_as_the_map(L, drive, tmp_path, fmt):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF)
    for f, (pts, stamp) in enumerate(drive[:4]):
        s.add_frame(pts, stamp, f)
    for m in (1, 3):
        pts, _ = L.dense_map(s, m)
        path = str(tmp_path / f"dense_{fmt}_{m}.pcd")
        assert L.save_dense_map_pcd(s, path, fmt, m) == pts.size > 100
        assert L.read_pcd(path).tobytes() == pts.tobytes()
    assert L.save_dense_map_pcd(s, str(tmp_path / "none.pcd"), fmt, 99) == 0 and not os.path.exists(str(tmp_path / "none.pcd"))
    s.close()
