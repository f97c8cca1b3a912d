"""The keypoint maps as PCD files on the device path: lsa_device_grid_add_pcd / _save_pcd (k_pcd_decode / k_pcd_encode) against
the oracle's RollingGrid and the independent PCD reader / writer of tests/pcd_cases.py, byte for byte; the pipeline calls
(lsa_slam_load_maps_pcd / _save_maps_pcd / _add_map_points) on device and host maps; localization in a loaded map against
the oracle session the map came from."""
import numpy as np
import pytest

import lidarslam_amd as L
import pcd_cases as P
from conftest import pose_diff
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GRID = dict(GridSize=12, VoxelResolution=8.0, LeafSize=0.2)  # 96 m wide: the far points of the cloud fall outside after the roll
LOAD_TIME = 1697500000.0


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def clouds():
    """Keyframes of an HDL-64 at three poses a step apart, stacked in WORLD: many points share a leaf voxel, within a
    keyframe and across them; a further frame for the ordinary Add that follows the load."""
    parts = []
    for f in (0, 1, 2):
        pts, _ = L.synth_frame(64, 1000, f)
        parts.append(O.transform(pts, L.synth_pose(f)))
    cloud = np.concatenate(parts)
    cloud["label"] = np.arange(cloud.size) % 7
    more = O.transform(L.synth_frame(64, 1000, 4)[0], L.synth_pose(4))
    assert cloud.size > 300000
    return cloud, more


@pytest.fixture(scope="module")
def files(clouds, tmp_path_factory):
    """the cloud written once per format by the helper.  CENTROID sampling takes the whole cloud too where the load is fixed; where
    it is not, the reference's CENTROID loop (restated by the oracle) takes a time that grows with the square of the points of a
    call -- a minute and more on the whole cloud, half a second on every sixteenth point, 24 506: still several workgroups,
    sort runs and points per voxel -- and those two configurations run on that"""
    d = tmp_path_factory.mktemp("map_io")
    out = {}
    for fmt in P.FORMATS:
        for thin in (0, 1):
            out[fmt, thin] = str(d / f"cloud_{fmt}_{thin}.pcd")
            P.write_points(out[fmt, thin], thinned(clouds[0], thin), fmt)
    return out


def thinned(cloud, thin):
    return cloud[::16] if thin else cloud


def thin_case(sampling, fixed):
    return sampling == 4 and not fixed


def box_of(pts):
    q = pts[:: 37]
    mn = np.array([q["x"].min() * 0.5, q["y"].min() * 0.5, q["z"].min()], np.float32)
    mx = np.array([q["x"].max() * 0.5, q["y"].max() * 0.5, q["z"].max()], np.float32)
    return mn, mx


_expected = {}


def expected_states(clouds, sampling, fixed, ordered):
    """the oracle grid that took the cloud as one Add, and then a further frame: computed once per configuration"""
    key = (sampling, fixed, ordered)
    if key not in _expected:
        cloud, more = thinned(clouds[0], thin_case(sampling, fixed)), (clouds[1][::8] if sampling == 4 else clouds[1])
        o = O.RollingGrid(Ordered=ordered, Sampling=sampling, MinFramesPerVoxel=2, **GRID)
        o.add(cloud, fixed=bool(fixed), time=LOAD_TIME, roll=True)
        mn, mx = box_of(clouds[0])
        first = dict(size=o.size(), all=o.get().tobytes(), clean=o.get(clean=True).tobytes(), sub_n=o.build_submap(mn, mx, 100), sub=None)
        first["sub"] = o.submap().tobytes()
        o.add(more, fixed=False, time=LOAD_TIME + 1, roll=True)
        second = dict(size=o.size(), all=o.get().tobytes(), clean=o.get(clean=True).tobytes())
        _expected[key] = (first, second)
    return _expected[key]


def device_grid(ctx, sampling, ordered):
    g = L.DeviceGrid(ctx)
    g.set("Ordered", ordered)  # before the first insertion: exact from then on
    for k, v in dict(Sampling=sampling, MinFramesPerVoxel=2, **GRID).items():
        g.set(k, v)
    return g


@pytest.mark.parametrize("ordered", [1, 0])
@pytest.mark.parametrize("fmt", P.FORMATS)
@pytest.mark.parametrize("fixed", [0, 1])
@pytest.mark.parametrize("sampling", [0, 1, 2, 3, 4])
def test_a_loaded_file_is_the_oracle_grid_byte_for_byte(ctx, clouds, files, sampling, fixed, fmt, ordered):
    cloud, more = thinned(clouds[0], thin_case(sampling, fixed)), (clouds[1][::8] if sampling == 4 else clouds[1])
    first, second = expected_states(clouds, sampling, fixed, ordered)
    g = device_grid(ctx, sampling, ordered)
    g.add_pcd(files[fmt, int(thin_case(sampling, fixed))], fixed=bool(fixed), time=LOAD_TIME, roll=True)
    assert g.size() == first["size"]
    assert 0 < first["size"] < cloud.size // 2  # points share voxels ...
    mn, mx = box_of(clouds[0])
    assert g.get().tobytes() == first["all"]
    assert g.get(clean=True).tobytes() == first["clean"]
    assert g.build_submap(mn, mx, 100) == first["sub_n"] > 0
    assert ctx.target(L.PLANE).tobytes() == first["sub"]
    # an ordinary Add afterwards: fixed voxels refuse it, the others take it and count it
    g.add(more, fixed=False, time=LOAD_TIME + 1, roll=True)
    assert g.size() == second["size"]
    assert g.get().tobytes() == second["all"]
    assert g.get(clean=True).tobytes() == second["clean"]
    after = np.frombuffer(second["all"], L.POINT_DTYPE)
    assert (after["time"] == LOAD_TIME + 1).any()  # the further frame did go in, at least into voxels of its own
    if fixed:
        assert (after["label"][after["time"] == LOAD_TIME] == 1).all() and (after["time"] == LOAD_TIME).sum() > 1000
    g.close()


def test_some_points_fall_outside_the_grid(clouds):
    cloud, _ = clouds
    o = O.RollingGrid(Sampling=0, **GRID)
    o.add(cloud, time=0.0)
    inside = o.get()
    half = GRID["GridSize"] * GRID["VoxelResolution"] / 2
    centre = np.array([(cloud[f].min() + cloud[f].max()) / 2 for f in "xyz"])
    assert (np.abs(cloud["x"] - centre[0]) > half + GRID["VoxelResolution"]).sum() > 100
    assert np.abs(inside["x"] - centre[0]).max() <= half + GRID["VoxelResolution"]


@pytest.mark.parametrize("ordered", [1, 0])
@pytest.mark.parametrize("clean", [0, 1])
@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_a_saved_map_is_the_oracle_get_bit_for_bit(ctx, clouds, tmp_path, fmt, clean, ordered):
    cloud, more = clouds
    g = device_grid(ctx, 2, ordered)
    o = O.RollingGrid(Ordered=ordered, Sampling=2, MinFramesPerVoxel=2, **GRID)
    for m in (g, o):
        m.add(cloud[:150001], time=1.0)
        m.add(cloud[100000:250001], time=2.0)  # the voxels both clouds touch have been seen twice: they pass the filter
        m.add(more, time=3.0)
    expected = o.get(clean=bool(clean))
    path = str(tmp_path / "saved.pcd")
    assert g.save_pcd(path, fmt, clean=bool(clean)) == expected.size > 1000
    fields, cols, name = P.read(path)
    assert name == P.FORMATS[fmt] and [f[0] for f in fields] == [f[0] for f in P.POINT_FIELDS]
    assert P.same_bits(P.to_points(cols, L.POINT_DTYPE), expected)
    # an empty map writes no file
    g.clear()
    empty = str(tmp_path / "empty.pcd")
    assert g.save_pcd(empty, fmt) == 0 and not (tmp_path / "empty.pcd").exists()
    g.close()


@pytest.mark.parametrize("lds", [0, 1])
# around a workgroup, and around a piece: 8 MiB hold 299 593 records of 28 bytes, rounded down to whole workgroups: 299 520 points
@pytest.mark.parametrize("n", [1, 255, 256, 257, 299519, 299520, 299521])
def test_both_forms_of_the_kernels_at_the_sizes_where_a_piece_ends(ctx, clouds, tmp_path, n, lds):
    cloud, _ = clouds
    part = cloud[:n]
    ctx.debug_set("pcd_lds", lds)
    try:
        g = device_grid(ctx, 0, 1)
        g.set("LeafSize", 0.02)  # most points a voxel of their own: little hides behind the sampling
        path = str(tmp_path / "in.pcd")
        P.write_points(path, part, "binary")
        g.add_pcd(path, time=0.0)
        o = O.RollingGrid(Sampling=0, **dict(GRID, LeafSize=0.02))
        o.add(part, time=0.0)
        assert g.get().tobytes() == o.get().tobytes()
        out = str(tmp_path / "out.pcd")
        assert g.save_pcd(out, 1) == o.size()
        assert P.same_bits(P.read_points(out, L.POINT_DTYPE), o.get())
        g.close()
    finally:
        ctx.debug_set("pcd_lds", -1)


def test_a_foreign_layout_is_decoded_on_the_device_as_on_the_host(ctx, clouds, tmp_path):
    """permuted fields, doubles for the coordinates, a byte for the intensity, an extra field, a vector field, no time: records of
    an odd size whose fields sit at unaligned offsets, as records and as columns"""
    cloud, _ = clouds
    n = 70001
    part = cloud[:n]
    rng = np.random.default_rng(5)
    columns = {"x": part["x"].astype(np.float64), "y": part["y"].astype(np.float64), "z": part["z"].astype(np.float64), "intensity": part["intensity"].astype(np.uint8),
               "laser_id": part["laser_id"].astype(np.int32), "label": part["label"], "normal_x": rng.standard_normal(n), "rgb": rng.standard_normal((n, 3))}
    fields = [("label", "I", 1, 1), ("rgb", "F", 4, 3), ("z", "F", 8, 1), ("normal_x", "F", 4, 1), ("intensity", "U", 1, 1), ("x", "F", 8, 1), ("y", "F", 8, 1), ("laser_id", "I", 4, 1)]
    for fmt in ("binary", "binary_compressed", "ascii"):
        m = n if fmt != "ascii" else 5001
        path = str(tmp_path / f"foreign_{fmt}.pcd")
        P.write(path, {k: v[:m] for k, v in columns.items()}, fields, fmt)
        expected = P.read_points(path, L.POINT_DTYPE)
        assert P.same_bits(L.read_pcd(path), expected)
        g = device_grid(ctx, 0, 1)
        g.add_pcd(path, time=3.0)
        o = O.RollingGrid(Sampling=0, **GRID)
        o.add(expected, time=3.0)
        assert g.get().tobytes() == o.get().tobytes() and g.size() > 1000
        g.close()


def test_a_malformed_file_is_refused_and_leaves_the_map_alone(ctx, clouds, tmp_path):
    cloud, _ = clouds
    good = str(tmp_path / "good.pcd")
    P.write_points(good, cloud[:1000], "binary")
    blob = open(good, "rb").read()
    bad = str(tmp_path / "short.pcd")
    open(bad, "wb").write(blob[:-7])
    g = device_grid(ctx, 2, 1)
    g.add_pcd(good, time=0.0)
    before = g.get().tobytes()
    with pytest.raises(L.LsaError, match="short.pcd"):
        g.add_pcd(bad, time=1.0)
    with pytest.raises(L.LsaError, match="nothing.pcd"):
        g.add_pcd(str(tmp_path / "nothing.pcd"), time=1.0)
    assert g.get().tobytes() == before
    g.close()


# ---------------------------------------------------------------------------------------- the pipeline
PARAMS = dict(EgoMotion=3, VoxelGridMinFramesPerVoxel=1)
# what a map point carries of the keypoint it was; its label and time are the Add's (fixed, current time: RollingGrid.cxx:226-227)
CONTENT = ["x", "y", "z", "intensity", "laser_id", "device_id"]


def sorted_points(pts, fields=None):
    a = np.ascontiguousarray(pts if fields is None else pts[fields])
    if fields is not None:
        packed = np.zeros(a.size, [(f, a.dtype[f]) for f in fields])
        for f in fields:
            packed[f] = a[f]
        a = packed
    return np.sort(a.view(f"V{a.dtype.itemsize}"))


# A session that goes on (the oracle's A) and a fresh one (B) must be in the same state when the first localized frame arrives.
# SetWorldTransformFromGuess (Slam.cxx:490-501) resets the pose, the previous pose and the previous keypoints, but not the
# trajectory log, and the log feeds two things a fresh session does without: the motion extrapolation of ComputeEgoMotion
# (:821-836, needs two logged poses: B has none, then one) and the undistortion's InterpolateScanPose (:1271-1285, an empty log
# means no motion within the frame).  With both on, A and B legitimately differ: 0.175 m / 8.3e-3 rad (VLP-16) and 0.145 m /
# 7.8e-4 rad (HDL-64) on the first localized frame, measured with EgoMotion = 3 and the default REFINED undistortion -- the
# reference's own behaviour on both sides, not an error of the loader.  So the sessions run with ego-motion by REGISTRATION
# alone and no undistortion: nothing then reads the log, and the bounds below hold frame by frame.
PRIOR = dict(EgoMotion=2, Undistortion=0, VoxelGridMinFramesPerVoxel=1)


@pytest.fixture(scope="module")
def prior_map_sessions(tmp_path_factory):
    """per sensor: oracle session A maps N frames, is told its own pose, and localizes frames N+1..M with the map frozen; its maps
    as they were at frame N are written by the helper.  N and M: A alone matches more than the pipeline tests' 1000 keypoints
    on every localized frame (VLP-16: 4111 and more; HDL-64: 15277 and more)."""
    out = {}
    for model, N, M in ((16, 8, 12), (64, 5, 8)):
        a = O.Slam(**PRIOR)
        for f in range(N + 1):
            pts, stamp = L.synth_frame(model, 1000, f)
            a.add_frame(pts, stamp, f)
        pose = a.world_transform()
        maps = [a.map(k, clean=False) for k in range(2)]
        a.set_world_transform_from_guess(pose)
        a.set_param("MapUpdate", 0)
        poses, submaps, matched = [], [], []
        for f in range(N + 1, M + 1):
            pts, stamp = L.synth_frame(model, 1000, f)
            a.add_frame(pts, stamp, f)
            poses.append(a.world_transform())
            submaps.append([a.submap(k) for k in range(2)])
            matched.append(a.stats()[12])
        prefix = str(tmp_path_factory.mktemp(f"prior_{model}") / "a_")
        for k, name in enumerate(("edges", "planes")):
            P.write_points(f"{prefix}{name}.pcd", maps[k], "binary")
        out[model] = dict(N=N, M=M, pose=pose, maps=maps, poses=poses, submaps=submaps, matched=matched, prefix=prefix)
    return out


@pytest.mark.parametrize("model", [16, 64])
def test_localizing_in_a_loaded_map_follows_the_oracle(prior_map_sessions, model):
    s = prior_map_sessions[model]
    assert min(s["matched"]) > 1000, s["matched"]
    b = L.Slam(0, MapUpdate=0, **PRIOR)
    counts = b.load_maps_pcd(s["prefix"], time=LOAD_TIME)
    assert counts == [s["maps"][0].size, s["maps"][1].size, -1]
    for k in range(2):  # every voxel of the file is a voxel of the map; RollingGrid::Add stamps label (fixed) and time (of the Add)
        got = b.map(k)
        assert np.array_equal(sorted_points(got, CONTENT), sorted_points(s["maps"][k], CONTENT))
        assert (got["label"] == 1).all() and (got["time"] == LOAD_TIME).all()
    b.set_world_transform_from_guess(s["pose"])
    worst = (0.0, 0.0)
    same_order = True
    for i, f in enumerate(range(s["N"] + 1, s["M"] + 1)):
        pts, stamp = L.synth_frame(model, 1000, f)
        b.add_frame(pts, stamp, f)
        dp, da = pose_diff(s["poses"][i], b.world_transform())
        worst = (max(worst[0], dp), max(worst[1], da))
        print(f"model {model} frame {f}: pose deviation {dp:.3e} m {da:.3e} rad")
        for k in range(2):
            sub = b.target_submap(k)
            assert np.array_equal(sorted_points(sub, CONTENT), sorted_points(s["submaps"][i][k], CONTENT)), (f, k)
            same_order = same_order and all(np.array_equal(sub[c], s["submaps"][i][k][c]) for c in CONTENT)
        # the loaded grid is centred on the cloud, the oracle's where it rolled: the same points, maybe in another order --
        # the bounds of tests/test_gpu_reference_map_order.py
        assert dp < 1e-7 and da < 1e-6, f"frame {f}: poses drift apart ({dp} m, {da} rad)"
    print(f"model {model}: sub-maps in the same order: {same_order}; largest deviation {worst[0]:.3e} m {worst[1]:.3e} rad")
    assert b.map(0).size == s["maps"][0].size  # MapUpdate = NONE: nothing was added
    b.close()


@pytest.fixture(scope="module")
def mapped_session():
    b = L.Slam(0, **PARAMS)
    for f in range(5):
        pts, stamp = L.synth_frame(16, 1000, f)
        b.add_frame(pts, stamp, f)
    yield b
    b.close()


def test_device_and_host_maps_load_the_same_files(mapped_session, tmp_path):
    prefix = str(tmp_path / "m_")
    counts = mapped_session.save_maps_pcd(prefix, L.PCD_BINARY, filtered=False)
    assert counts[0] > 100 and counts[1] > 1000 and counts[2] == -1 and not (tmp_path / "m_blobs.pcd").exists()
    dev, host = L.Slam(0, **PARAMS), L.Slam(0, MapsOnDevice=0, **PARAMS)
    assert dev.get_param("DeviceMapsInUse") == 1.0 and host.get_param("DeviceMapsInUse") == 0.0
    for s in (dev, host):
        assert s.load_maps_pcd(prefix, time=LOAD_TIME) == counts
    for k in range(3):
        assert dev.map(k).tobytes() == host.map(k).tobytes()
        assert dev.map(k, clean=True).tobytes() == host.map(k, clean=True).tobytes()
    # and what the host-maps session saves is what the device-maps session saves; every voxel was seen once, and Get(clean) wants
    # more than MinFramesPerVoxel = 1: the filtered maps are empty and write nothing
    for s, name in ((dev, "d_"), (host, "h_")):
        assert s.save_maps_pcd(str(tmp_path / ("f" + name)), L.PCD_BINARY, filtered=True) == [-1, -1, -1]
        assert s.save_maps_pcd(str(tmp_path / name), L.PCD_BINARY_COMPRESSED, filtered=False) == counts
    assert not list(tmp_path.glob("fd_*")) and not list(tmp_path.glob("fh_*"))
    for f in ("edges.pcd", "planes.pcd"):
        assert P.same_bits(P.read_points(str(tmp_path / ("d_" + f)), L.POINT_DTYPE), P.read_points(str(tmp_path / ("h_" + f)), L.POINT_DTYPE))
    dev.close()
    host.close()


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_round_trip_through_the_pipeline(mapped_session, tmp_path, fmt):
    b = mapped_session
    prefix = str(tmp_path / "rt_")
    b.save_maps_pcd(prefix, fmt, filtered=False)
    c = L.Slam(0, MapUpdate=0, **PARAMS)
    c.add_map_points(L.PLANE, b.map(L.PLANE)[:10], fixed=False, time=1.0)  # reset_maps = 1 throws these away
    c.load_maps_pcd(prefix, reset_maps=True, time=LOAD_TIME)
    for k in range(2):
        got, want = c.map(k), b.map(k)
        assert got.size == want.size > 100
        assert np.array_equal(sorted_points(got, CONTENT), sorted_points(want, CONTENT))
        assert (got["label"] == 1).all() and (got["time"] == LOAD_TIME).all()  # fixed (MapUpdate = NONE), stamped with the load
    c.close()


def test_loading_onto_maps_that_hold_points(mapped_session, tmp_path):
    """reset_maps = 0: the map is the oracle grid that received both Adds (the second one fixed: MapUpdate = NONE)"""
    b = mapped_session
    prefix = str(tmp_path / "two_")
    b.save_maps_pcd(prefix, L.PCD_BINARY, filtered=False)
    first = O.transform(L.synth_frame(16, 1000, 9)[0][::5], L.synth_pose(9))
    for on_device in (1, 0):
        c = L.Slam(0, MapUpdate=0, MapsOnDevice=on_device, **PARAMS)
        for k in range(2):
            c.add_map_points(k, first, fixed=False, time=5.0)
        c.load_maps_pcd(prefix, reset_maps=False, time=LOAD_TIME)
        for k in range(2):
            o = O.RollingGrid(VoxelResolution=10.0, GridSize=50, LeafSize=c.get_param("VoxelGridLeafSizeEdges" if k == 0 else "VoxelGridLeafSizePlanes"), Sampling=2, MinFramesPerVoxel=1)
            o.add(first, fixed=False, time=5.0)
            o.add(P.read_points(prefix + ("edges.pcd" if k == 0 else "planes.pcd"), L.POINT_DTYPE), fixed=True, time=LOAD_TIME)
            assert c.map(k).tobytes() == o.get().tobytes(), (on_device, k)
            assert c.map(k, clean=True).tobytes() == o.get(clean=True).tobytes(), (on_device, k)
        c.close()


@pytest.mark.parametrize("on_device", [1, 0])
@pytest.mark.parametrize("filtered", [True, False])
def test_a_prefix_that_cannot_be_written_is_an_error(tmp_path, on_device, filtered):
    """a map that is not saved must say so: on both homes of the maps, filtered or not, naming the file"""
    s = L.Slam(0, MapsOnDevice=on_device, **PARAMS)
    for f in range(3):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
    assert s.map(L.PLANE, clean=True).size > 100  # there is something to save, also behind the filter
    with pytest.raises(L.LsaError, match=r"no_such_directory/m_(edges|planes)\.pcd"):
        s.save_maps_pcd(str(tmp_path / "no_such_directory" / "m_"), L.PCD_BINARY, filtered=filtered)
    assert sum(c > 0 for c in s.save_maps_pcd(str(tmp_path / "m_"), L.PCD_BINARY, filtered=filtered)) == 2  # and the session is none the worse
    s.close()


def test_a_grid_that_cannot_write_its_file_says_so(ctx, clouds, tmp_path):
    g = device_grid(ctx, 2, 1)
    g.add(clouds[0][:5000], time=0.0)
    for fmt in (0, 1, 2):
        with pytest.raises(L.LsaError, match="missing/map.pcd"):
            g.save_pcd(str(tmp_path / "missing" / "map.pcd"), fmt)
    assert g.save_pcd(str(tmp_path / "map.pcd"), 1) == g.size() > 100
    g.close()


def test_a_missing_prefix_loads_nothing_and_a_broken_file_is_an_error(tmp_path):
    c = L.Slam(0, **PARAMS)
    assert c.load_maps_pcd(str(tmp_path / "none_"), time=0.0) == [-1, -1, -1]
    open(str(tmp_path / "bad_planes.pcd"), "wb").write(b"VERSION 0.7\nFIELDS x y z\nSIZE 4 4\nTYPE F F F\nWIDTH 1\nHEIGHT 1\nPOINTS 1\nDATA ascii\n0 0 0\n")
    with pytest.raises(L.LsaError, match="bad_planes.pcd"):
        c.load_maps_pcd(str(tmp_path / "bad_"), time=0.0)
    assert c.save_maps_pcd(str(tmp_path / "empty_")) == [-1, -1, -1]  # empty maps write nothing
    assert not list(tmp_path.glob("empty_*"))
    c.close()
