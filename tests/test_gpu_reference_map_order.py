"""The reference's map point order on the device maps ("Ordered" = 0 on lsa_device_grid, "OrderedMaps" = 0 on lsa_slam).

The reference's RollingGrid::Get / BuildSubMapKdTree hand the points out in the iteration order of its
unordered_map<int, unordered_map<int, Voxel>> (RollingGrid.cxx:95-113, 362-442).  The device grid records what every
modification did to its key set, the host replays that on a keys-only copy of those containers, and the extractions
compact over the order the copy gives.  Checked here against the oracle's restatement of RollingGrid.cxx with the same
switch ("Ordered" = 0, the yardstick): maps, clean maps and sub-maps byte for byte, poses within the bounds of
tests/test_gpu_pipeline.py's run_both."""
import numpy as np
import pytest

import lidarslam_amd as L
import test_gpu_device_grid as base
from conftest import pose_diff
from oracle import oracle as O
from test_rolling_grid import cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def ordered_pair(ctx, **params):
    """a device grid and an oracle grid in the reference's container order, from their first insertion on"""
    g = L.DeviceGrid(ctx)
    g.set("Ordered", 0)
    for k, v in params.items():
        g.set(k, v)
    return g, O.RollingGrid(Ordered=0, **params)


@pytest.fixture
def reference_order(monkeypatch):
    """the scenarios of test_gpu_device_grid.py, both grids with "Ordered" = 0"""
    monkeypatch.setattr(base, "pair", ordered_pair)


# ---------------------------------------------------------------------------------------- the grid on its own
@pytest.mark.parametrize("sampling", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("min_frames", [0, 3])
def test_add_roll_and_submaps(ctx, reference_order, sampling, min_frames):
    base.test_add_roll_and_submaps_follow_the_oracle(ctx, sampling, min_frames)


def test_large_batches_and_many_keyframes(ctx, reference_order):
    base.test_large_batches_and_many_keyframes(ctx)


def test_the_box_of_an_empty_cloud_selects_nothing(ctx, reference_order):
    base.test_the_box_of_an_empty_cloud_selects_nothing(ctx)


def test_rolling_away(ctx, reference_order):
    base.test_rolling_away_drops_the_voxels_left_behind(ctx)


def test_decay_with_fixed_points(ctx, reference_order):
    base.test_decaying_threshold_and_fixed_points(ctx)


@pytest.mark.parametrize("n", [1, 255, 4096, 4097, 12289])
def test_batches_around_the_sort_sizes(ctx, reference_order, n):
    base.test_batches_around_the_sizes_the_sort_is_built_of(ctx, n)


def test_geometry_setters_reset_and_clear(ctx, reference_order):
    base.test_changing_the_geometry_puts_the_points_back(ctx)


def test_centroid_sampling(ctx, reference_order):
    base.test_centroid_sampling_with_the_reference_loop_quirk(ctx)


def test_keypoints_of_the_context(ctx, reference_order):
    base.test_keypoints_of_the_context_go_into_the_map_without_leaving_the_device(ctx)


def test_the_two_step_calls_from_another_thread(ctx, reference_order):
    base.test_the_two_step_calls_of_the_pipeline(ctx)


def test_the_order_is_the_containers_and_not_the_keys(ctx):
    """the same map in both orders: the same voxels, handed out in another order (or the checks above would show nothing)"""
    rng = np.random.default_rng(12)
    g0, o0 = ordered_pair(ctx, GridSize=20, VoxelResolution=6.0, LeafSize=0.5)
    g1 = L.DeviceGrid(ctx, GridSize=20, VoxelResolution=6.0, LeafSize=0.5)
    assert g0.get_param("Ordered") == 0.0 and g1.get_param("Ordered") == 1.0
    for step in range(4):
        pts = cloud(rng, 5000, np.array([step * 4.0, 0, 0]), spread=20.0, t=step * 0.1)
        for m in (g0, g1, o0):
            m.add(pts, time=step * 0.1)
    a, b = g0.get(), g1.get()
    assert a.tobytes() == o0.get().tobytes()
    assert a.size == b.size > 5000 and a.tobytes() != b.tobytes()
    voxels = lambda c: sorted(c.view(np.dtype((np.void, c.itemsize))).tolist())
    assert voxels(a) == voxels(b)
    g0.close(), g1.close()


def test_switching_the_order_on_a_grid_that_holds_points(ctx):
    """"Ordered" set while the grid holds points: the points, in the order they are handed out at that moment, go back into
    the emptied grid (Get, Clear, Add, as the geometry setters do); to the reference's order, into containers never used"""
    rng = np.random.default_rng(32)
    params = dict(GridSize=10, VoxelResolution=6.0, LeafSize=0.5, Sampling=1)
    g, o = L.DeviceGrid(ctx, **params), O.RollingGrid(**params)  # key order on both sides
    for step in range(3):
        pts = cloud(rng, 1500, np.array([step * 2.0, 0, 0]), spread=10.0, t=step * 0.1)
        g.add(pts, time=step * 0.1, roll=False), o.add(pts, time=step * 0.1, roll=False)  # the grid stays where Reset put it
    base.same_state(g, o)
    # key order -> the reference's order
    held = o.get()
    g.set("Ordered", 0)
    assert g.get_param("Ordered") == 0.0
    r = O.RollingGrid(Ordered=0, **params)  # containers never used, at the same place
    r.add(held)
    base.same_state(g, r)
    for step in range(3, 7):
        pts = cloud(rng, 1500, np.array([step * 6.0, 0, 0]), spread=10.0, t=step * 0.1)
        g.add(pts, time=step * 0.1), r.add(pts, time=step * 0.1)
        base.same_state(g, r)
        base.same_submap(g, r)
    # and back: the points in the reference's order, into the grid emptied, handed out in key order
    held = r.get()
    g.set("Ordered", 1)
    r.set("Ordered", 1)
    r.clear()
    r.add(held)
    base.same_state(g, r)
    base.same_submap(g, r)
    g.close()


# ---------------------------------------------------------------------------------------- the pipeline
def run_ordered(L, O, model, nframes, seed=1000, **params):
    """tests/test_gpu_pipeline.py's run_both with "OrderedMaps" = 0 on both sides"""
    params.setdefault("EgoMotion", 3)
    oracle_params = {k: v for k, v in params.items() if k != "MapsOnDevice"}
    sg, so = L.Slam(0, OrderedMaps=0, **params), O.Slam(OrderedMaps=0, **oracle_params)
    assert sg.get_param("OrderedMaps") == 0.0
    poses = []
    for f in range(nframes):
        pts, stamp = L.synth_frame(model, seed, f)
        sg.add_frame(pts, stamp, f)
        so.add_frame(pts, stamp, f)
        dp, da = pose_diff(so.world_transform(), sg.world_transform())
        assert dp < 1e-7 and da < 1e-6, f"frame {f}: poses drift apart ({dp} m, {da} rad)"
        poses.append(sg.world_transform())
    return sg, so, np.array(poses)


def same_maps(sg, so, types=range(3)):
    for k in types:
        assert sg.map(k).tobytes() == so.map(k).tobytes(), k
        assert sg.map(k, clean=True).tobytes() == so.map(k, clean=True).tobytes(), k
        assert sg.target_submap(k).tobytes() == so.submap(k).tobytes(), k


@pytest.mark.parametrize("model,nframes", [(16, 30), (64, 40), (128, 6)])
def test_pipeline_on_device_maps(L, O, model, nframes):
    """HDL-64 x 40 runs past frame 36, where key order takes another ICP decision than the reference's order"""
    sg, so, _ = run_ordered(L, O, model, nframes)
    same_maps(sg, so)
    assert sg.get_param("DeviceMapsInUse") == 1.0
    assert sg.get_param("DeviceSolveFallbacks") == 0.0
    sg.close()


@pytest.mark.parametrize("model,nframes", [(16, 30), (64, 40)])
def test_pipeline_on_host_maps(L, O, model, nframes):
    sg, so, _ = run_ordered(L, O, model, nframes, MapsOnDevice=0)
    same_maps(sg, so)
    assert sg.get_param("DeviceMapsInUse") == 0.0
    sg.close()


@pytest.mark.parametrize(
    "params",
    [
        dict(),
        dict(KfDistanceThreshold=1.2),
        dict(VoxelGridDecayingThreshold=0.45, VoxelGridMinFramesPerVoxel=2),
        dict(VoxelGridSamplingMode=1), dict(VoxelGridSamplingMode=3), dict(VoxelGridSamplingMode=4),
        dict(MapUpdate=0),
    ],
)
@pytest.mark.parametrize("on_device", [1, 0])
def test_map_maintenance(L, O, params, on_device):
    """the matrix of test_map_maintenance_beside_the_device_work, with the same assertions"""
    sg, so, poses = run_ordered(L, O, 8, 30, MapsOnDevice=on_device, **params)
    assert sg.get_param("DeviceMapsInUse") == (1.0 if on_device else 0.0)
    if params.get("MapUpdate", 2) != 0:
        decaying_on_device = on_device and "VoxelGridDecayingThreshold" in params
        assert (sg.get_param("SubMapSpeculationHits") > 0) == (not decaying_on_device)
    same_maps(sg, so)
    step = np.linalg.norm(poses[-1][:3, 3] - poses[10][:3, 3])
    assert step > 5.0 or params.get("MapUpdate", 2) == 0
    sg.close()


# ---------------------------------------------------------------------------------------- schedules and resets
def test_maps_moved_between_device_and_host(L):
    """"MapsOnDevice" set in the middle of a sequence: the points change sides in the order they are handed out, the
    sequence goes on close to the one that never switched, with the same number of map points right after each move"""
    ref = L.Slam(0, OrderedMaps=0, EgoMotion=3)
    sw = L.Slam(0, OrderedMaps=0, EgoMotion=3)
    for f in range(16):
        pts, stamp = L.synth_frame(8, 1000, f)
        if f in (6, 11):
            before = [sw.map(k).size for k in range(3)]
            sw.set_param("MapsOnDevice", 0 if f == 6 else 1)
            assert sw.get_param("DeviceMapsInUse") == (0.0 if f == 6 else 1.0)
            assert [sw.map(k).size for k in range(3)] == before and sum(before) > 500
        ref.add_frame(pts, stamp, f)
        sw.add_frame(pts, stamp, f)
        dp, da = pose_diff(ref.world_transform(), sw.world_transform())
        assert dp < 2e-2 and da < 2e-3, (f, dp, da)
    ref.close(), sw.close()


def test_sub_maps_ahead_change_nothing_but_the_schedule(L):
    a = L.Slam(0, OrderedMaps=0, EgoMotion=3, SubMapsAhead=1, SubMapsAheadAdaptive=0)
    b = L.Slam(0, OrderedMaps=0, EgoMotion=3, SubMapsAhead=0)
    for f in range(25):
        pts, stamp = L.synth_frame(16, 1000, f)
        for s in (a, b):
            s.add_frame(pts, stamp, f)
        assert np.array_equal(a.world_transform(), b.world_transform()), f
        for k in range(2):
            assert a.target_submap(k).tobytes() == b.target_submap(k).tobytes(), (f, k)
    for k in range(2):
        assert a.map(k).tobytes() == b.map(k).tobytes()
    assert a.get_param("SubMapSpeculationHits") > 20 and b.get_param("SubMapSpeculationHits") == 0
    a.close(), b.close()


def test_reset_then_a_second_pass(L, O):
    """Reset() empties the maps through clear(), which keeps the bucket arrays: the second pass's order is the oracle's
    second pass's (not necessarily its first's).  Nothing reads the maps between the first pass and the reset."""
    sg, so = L.Slam(0, OrderedMaps=0, EgoMotion=3), O.Slam(OrderedMaps=0, EgoMotion=3)
    for run in range(2):
        if run == 1:
            sg.reset(), so.reset()
        for f in range(14):
            pts, stamp = L.synth_frame(16, 1000, f)
            sg.add_frame(pts, stamp, f)
            so.add_frame(pts, stamp, f)
            dp, da = pose_diff(so.world_transform(), sg.world_transform())
            assert dp < 1e-7 and da < 1e-6, (run, f, dp, da)
    same_maps(sg, so)
    assert sg.get_param("DeviceMapsInUse") == 1.0
    sg.close()


@pytest.mark.parametrize("last", ["add", "roll", "decay"])
@pytest.mark.parametrize("how", ["reset", "clear"])
def test_emptied_right_after_a_modification(ctx, last, how):
    """reset / clear straight behind a modification, nothing read in between.  clear() keeps the outer table's bucket
    array, and the last modification decided its size: a wide insertion grows it to hundreds of outer voxels, a roll that
    leaves none behind replaces it by a fresh table.  The few outer voxels inserted after the clear are handed out in an
    order that depends on that size."""
    rng = np.random.default_rng(41 + len(last) + len(how))
    g, o = ordered_pair(ctx, GridSize=20, VoxelResolution=6.0, LeafSize=0.5, DecayingThreshold=0.15)
    small = cloud(rng, 2000, np.zeros(3), spread=4.0, t=0.0)
    g.add(small, time=0.0), o.add(small, time=0.0)
    wide = cloud(rng, 30000, np.zeros(3), spread=55.0, t=0.1)
    g.add(wide, time=0.1), o.add(wide, time=0.1)
    if last == "roll":
        mn, mx = np.full(3, 200.0, np.float32), np.full(3, 210.0, np.float32)  # the grid moves by more than its size
        g.roll(mn, mx), o.roll(mn, mx)
    elif last == "decay":
        g.clear_old_points(0.3), o.clear_old_points(0.3)
    if how == "reset":
        g.reset([1.0, 2.0, 3.0]), o.reset([1.0, 2.0, 3.0])
    else:
        g.clear(), o.clear()
    # (no roll: a roll that moves rebuilds the outer table.  Clear leaves the grid where the roll took it: 25 voxels on.)
    at = 150.0 if (last, how) == ("roll", "clear") else 0.0
    for step in range(2):
        pts = cloud(rng, 3000, np.array([at + step * 1.0, at, at]), spread=4.0, t=1.0 + step * 0.1)
        g.add(pts, time=1.0 + step * 0.1, roll=False), o.add(pts, time=1.0 + step * 0.1, roll=False)
    base.same_state(g, o)
    assert base.same_submap(g, o) > 500
    g.close()
