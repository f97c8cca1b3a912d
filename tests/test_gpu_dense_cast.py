"""Rays through the dense map on the device (lidarslam_amd/csrc/lsa_dense_cast.hip: k_dense_cast, k_dense_compare) against
DenseMapHost.cast / .compare, byte for byte on hit records, points, labels and counts, and on the count of rays; after every
call the map's state is what it was.  The walk's cases, ties, wavefront edges, the predicate, long probe sequences, growth,
prune, re-projection, clear, the fused frame path, the pipeline, the render, refusals.  Cases: tests/dense_cast_cases.py."""
import ctypes as C

import numpy as np
import pytest

import dense_carve_cases as K
import dense_cast_cases as R
import dense_map_cases as M
from conftest import two_device_rig
from test_gpu_dense_map import NFRAMES, PIPE_LEAF, frame_path, transform_frame_at

pytestmark = pytest.mark.gpu

INF = float("inf")


class Pair:
    """a device map and the host statement, fed alike; every cast and compare is held to the host's bytes and to an unchanged map"""

    def __init__(self, L, ctx, leaf=K.LEAF, **params):
        self.d = L.DenseMap(ctx, leaf, **params)
        self.h = L.DenseMapHost(leaf)

    def insert(self, pts, frame):
        self.d.insert_points(pts, frame)
        self.h.insert(pts, frame)

    def carve(self, pts, origins, frame):
        self.d.carve_points(pts, origins, frame)
        self.h.carve(pts, origins, frame)

    def unchanged(self, call):
        before = R.state(self.h)
        K.same_state(self.d, self.h)
        out = call()
        assert K.same_state(self.d, self.h) == self.h.size() and R.state(self.h) == before
        assert self.d.get_param("CastRays") == self.h.cast_rays and self.d.get_param("Rays") == self.h.rays
        return out

    def cast(self, origins, targets, **kw):
        def call():
            dh, dp = self.d.cast(origins, targets, **kw)
            hh, hp = self.h.cast(origins, targets, **kw)
            assert dh.dtype == hh.dtype and dh.tobytes() == hh.tobytes(), (dh[dh != hh][:4], hh[dh != hh][:4])
            assert dp.tobytes() == hp.tobytes()
            return hh
        return self.unchanged(call)

    def compare(self, pts, origins, **kw):
        def call():
            dl, dc = self.d.compare_points(pts, origins, **kw)
            hl, hc = self.h.compare(pts, origins, **kw)
            assert dl.dtype == hl.dtype == np.uint8 and dl.tobytes() == hl.tobytes() and dc.tolist() == hc.tolist()
            return hl
        return self.unchanged(call)

    def close(self):
        self.d.close()


# ---- 1. the walk ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.RAY_CASES))
def test_every_ray_case_as_one_call(L, gpu_ctx, name):
    o, t, kw = R.cast_case(name)
    p = Pair(L, gpu_ctx)
    p.insert(R.thinned_scene(name), 0)
    for extend in R.EXTENDS + (kw["extend"],):
        hit = p.cast(o, t, extend=extend, max_range=kw["max_range"])[0]
        if extend == kw["extend"]:
            assert (hit["status"] == -1) == (name in K.NO_RAY)
    empty = Pair(L, gpu_ctx)  # a map without a table: the whole walk, no hit
    hit = empty.cast(o, t, **kw)[0]
    assert hit["steps"] == (0 if name in K.NO_RAY else len(K.walk(name)))
    assert p.compare(K.cloud(t), o, tolerance=0.0, max_range=kw["max_range"]).size == 1
    p.close(), empty.close()


@pytest.mark.parametrize("name", sorted(K.TIES))
def test_ties(L, gpu_ctx, name):
    o, t, kw = R.cast_case(name)
    visited = K.TIES[name]
    for k in range(len(visited) - 1):
        here = np.array(visited[k])
        toward = np.sign(np.array(visited[-1]) - here)
        p = Pair(L, gpu_ctx)
        p.insert(K.voxel_points([tuple(here + toward * np.eye(3, dtype=np.int64)[a]) for a in range(3) if toward[a] != 0]), 0)
        hit = p.cast(o, t, **kw)[0]
        assert (hit["status"], hit["steps"], hit["key"]) == (1, k + 2, R.key_of(visited[k + 1]))
        p.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_wavefront_edges(L, gpu_ctx, n):
    targets = R.xyz(K.ray_cloud(n, seed=n))
    org = np.random.default_rng(n).uniform(-1, 1, (n, 3)).astype(np.float32)
    p = Pair(L, gpu_ctx)
    p.insert(K.ray_cloud(4097, seed=7), 0)
    hits = np.concatenate([p.cast(org, targets), p.cast(org[:1], targets, extend=INF, max_range=8.0)])
    labels = np.concatenate([p.compare(K.ray_cloud(n, seed=n), org), p.compare(K.ray_cloud(n, seed=n), org[:1], tolerance=0.0)])
    assert (hits["status"] >= 0).all() and (labels != 0).all()
    if n == 4097:
        assert set(hits["status"].tolist()) == {0, 1} and set(labels.tolist()) == {1, 2, 3}
    p.close()


def test_one_wavefront_of_no_steps_early_hits_late_hits_and_misses(L, gpu_ctx):
    pts, org, leaf, max_range = K.mixed_wavefront()
    walks = R.cast_walks(org, R.xyz(pts), leaf, extend=0.0, max_range=max_range)
    assert [len(w) for w in walks[::2]] == [1] * 32 and min(len(w) for w in walks[1::2]) > 4096
    # every fifth voxel of the long walks of the odd lanes 1, 5, 9, ...; from a different depth in each
    along = np.concatenate([np.asarray([v for v, _, _ in walks[lane][64 * lane + 3::5]]) for lane in range(1, 64, 4)])
    p = Pair(L, gpu_ctx, leaf=leaf)
    p.insert(K.voxel_points(np.unique(along, axis=0), leaf=leaf), 0)
    hits = p.cast(org, R.xyz(pts), extend=0.0, max_range=max_range)
    assert (hits["steps"][::2] == 1).all() and (hits["status"][1::4] == 1).all() and hits["steps"][1::4].min() < 100 < 3000 < hits["steps"][1::4].max()
    assert (hits["status"][3::4] == 0).sum() > 8 and hits["steps"].max() > 4096
    p.compare(pts, org, tolerance=leaf, max_range=max_range)
    p.close()


# ---- 2. the predicate, and the table in its other states --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def carved(L, gpu_ctx):
    h, wall, obj = K.host_scene()
    d, _, _ = K.carved_scene(lambda: L.DenseMap(gpu_ctx, K.LEAF))
    p = Pair.__new__(Pair)
    p.d, p.h = d, h
    yield p, K.voxel_points(wall)
    d.close()


@pytest.mark.parametrize("min_frames", [1, 2, 8])
@pytest.mark.parametrize("ratio", K.RATIOS)
@pytest.mark.parametrize("before", [None, 4])
def test_the_predicate_on_the_carved_scene(carved, min_frames, ratio, before):
    p, wall = carved
    hits = p.cast(K.SENSOR, R.xyz(wall), extend=K.LEAF, min_frames=min_frames, max_miss_ratio=ratio, before=before)
    labels = p.compare(wall, K.SENSOR, min_frames=min_frames, max_miss_ratio=ratio, before=before)
    assert (hits["status"] == 1).all() and (labels != 0).all()  # the wall itself passes every one of these predicates
    if ratio < 0 and min_frames == 1:
        assert (hits["steps"] < 12).sum() > 0  # rays that end in the object, half way to the wall


def test_probe_stress_gives_the_same_hits(L, gpu_ctx):
    pts, targets = K.ray_cloud(700, seed=3), R.xyz(K.ray_cloud(300, seed=4, reach=9.0))
    org = np.zeros((1, 3), np.float32)
    stressed, plain = Pair(L, gpu_ctx, InitialCapacity=64, ProbeStress=1), Pair(L, gpu_ctx)
    got = []
    for p in (stressed, plain):
        p.insert(pts[:400], 0)
        p.insert(pts[400:], 2)
        got.append(p.cast(org, targets, extend=1.0).tobytes() + p.compare(K.ray_cloud(300, seed=4, reach=9.0), org).tobytes())
    assert stressed.d.get_param("Rehashes") >= 1 and got[0] == got[1]
    stressed.close(), plain.close()


def test_after_growth_prune_reproject_and_clear(L, gpu_ctx):
    calls = M.growth_calls()
    org = np.array([[0.3, -0.2, 0.1]], np.float32)
    p = Pair(L, gpu_ctx, InitialCapacity=64)
    for pts, frame in calls[:3]:
        p.insert(pts, 2 * frame)
    rays = calls[4][0][::7]
    p.carve(rays, org, 5)
    before = p.d.get_param("Rehashes")
    p.cast(org, R.xyz(rays), extend=INF, max_range=12.0)
    for pts, frame in calls[3:]:
        p.insert(pts, 2 * frame)  # the table doubles under these
    assert p.d.get_param("Rehashes") > before
    hits = p.cast(org, R.xyz(rays), extend=INF, max_range=12.0, max_miss_ratio=0.5)
    p.compare(rays, org, max_miss_ratio=0.5)
    assert (hits["status"] == 1).sum() > 10
    assert p.d.prune(2, -1.0) == p.h.prune(2, -1.0)
    p.cast(org, R.xyz(rays), extend=INF, max_range=12.0)
    D = np.stack([np.eye(4)] * 12)
    D[1::2, 1, 3] = 0.5
    assert p.d.reproject(D) == p.h.reproject(D.reshape(-1, 16))
    p.cast(org, R.xyz(rays), extend=INF, max_range=12.0)
    p.compare(rays, org)
    assert p.h.cast_rays > 0
    p.d.clear(), p.h.clear()
    hits = p.cast(org, R.xyz(rays), extend=INF, max_range=12.0)
    assert (hits["status"] == 0).all() and p.d.get_param("CastRays") == len(rays)  # every ray misses, and the count restarts
    p.close()


# ---- 3. the fused path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interpolate", [False, True])
@pytest.mark.parametrize("time_offset", [0.0, 0.0125])
def test_compare_frame_is_compare_points_of_the_transformed_frame_and_its_origins(L, gpu_ctx, interpolate, time_offset):
    leaf = 0.2
    p = Pair(L, gpu_ctx, leaf=leaf)
    kw = dict(max_range=15.0)
    for f in range(3):
        pts, _ = L.synth_frame(16, 1000, f)
        gpu_ctx.upload_frame(pts)
        H0, H1 = L.synth_pose(f), (L.synth_pose(f + 1) if interpolate else None)
        world = transform_frame_at(L, gpu_ctx, H0, H1, -0.1, 0.0, time_offset)
        origins = L.frame_origins_at(gpu_ctx, H0, H1, -0.1, 0.0, time_offset)
        if f == 2:  # against the map of the two frames before
            rays = p.h.cast_rays
            host = p.compare(world, origins, **kw)
            fused, counts = p.d.compare_frame(H0, H1, -0.1, 0.0, time_offset, **kw)
            assert fused.tobytes() == host.tobytes() and counts.tolist() == np.bincount(host, minlength=4).tolist()
            assert p.d.get_param("CastRays") == rays + 2 * (p.h.cast_rays - rays)
            assert (host == 1).sum() > (host != 0).sum() // 2 and (host == 2).sum() > 0 and (host == 0).sum() > 0
            K.same_state(p.d, p.h)
        p.d.insert_frame(f, H0, H1, -0.1, 0.0, time_offset)
        p.h.insert(world, f)
    p.close()


def test_a_frame_uploaded_in_wire_format_waits_for_the_compare_that_reads_its_buffer(L):
    """the case of tests/test_gpu_dense_carve.py with a compare_frame as the last reader of the frame's buffer"""
    from test_gpu_pipeline import VELODYNE_LAYOUT, wire_records

    leaf = 0.2
    ctx = L.Context(0)
    d, h = L.DenseMap(ctx, leaf), L.DenseMapHost(leaf)
    got, worlds = [], []
    for f in range(4):
        pts, _ = L.synth_frame(16, 1000, f)
        ctx.upload_wire_frame(wire_records(pts), VELODYNE_LAYOUT)
        H0, H1 = L.synth_pose(f), L.synth_pose(f + 1)
        worlds.append((transform_frame_at(L, ctx, H0, H1, -0.1, 0.0, 0.0), L.frame_origins_at(ctx, H0, H1, -0.1, 0.0)))
        d.insert_frame(f, H0, H1, -0.1, 0.0)
        got.append(d.compare_frame(H0, H1, -0.1, 0.0, max_range=15.0, before=f))  # the next upload follows at once
    for f, (world, origins) in enumerate(worlds):
        h.insert(world, f)
        labels, counts = h.compare(world, origins, max_range=15.0, before=f)
        assert got[f][0].tobytes() == labels.tobytes() and got[f][1].tolist() == counts.tolist()
    assert (got[3][0] == 1).sum() > 5000
    K.same_state(d, h)
    d.close()
    ctx.close()


# ---- 4. the pipeline -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drive(L):
    return [L.synth_frame(16, 1000, f) for f in range(NFRAMES)]


def pipeline(L, drive, calls, box_at=None, **params):
    """the drive through a pipeline with the dense map on; at the frames of `calls` the labels of dense_map_compare_frame are held
    to the host statement.  -> (slam, host map, {frame: labels})"""
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, DenseMapCarve=1, DenseMapCarveRange=12.0, DenseMapCarveStride=3, **params)
    h = L.DenseMapHost(PIPE_LEAF)
    out = {}
    for f, (pts, stamp) in enumerate(drive):
        if f == box_at:
            pts = np.concatenate([pts, R.box_points()])
        s.add_frame(pts, stamp, f)
        if f in calls:
            world, origins = s.registered_frame().copy(), L.registered_frame_origins(s)
            h.insert(world, f)
            labels, counts = L.dense_map_compare_frame(s)
            hl, hc = h.compare(world, origins, before=f)
            assert labels.tobytes() == hl.tobytes() and counts.tolist() == hc.tolist() and len(labels) == world.size
            out[f] = labels
        elif calls:
            h.insert(s.registered_frame(), f)
    return s, h, out


def test_the_pipelines_labels_are_the_host_statement_and_the_frame_path_does_not_notice(L, drive):
    quiet, _, _ = pipeline(L, drive, ())
    path = frame_path(L, quiet)
    voxels = L.dense_map_filtered(quiet, 1, -1.0)[1].tobytes(), L.dense_map_misses(quiet).tobytes(), quiet.get_param("DenseMapRays")
    quiet.close()
    s, h, labels = pipeline(L, drive, (4, 8, 11))
    for f, lab in labels.items():
        judged = lab != 0
        assert (lab[judged] == 1).sum() > judged.sum() // 2, f  # more than half the judged points are CONSISTENT
    assert frame_path(L, s) == path
    assert (L.dense_map_filtered(s, 1, -1.0)[1].tobytes(), L.dense_map_misses(s).tobytes(), s.get_param("DenseMapRays")) == voxels
    # explicit ordinals and none at all; a scan of the map from here; the map's own call
    world, origins = s.registered_frame().copy(), L.registered_frame_origins(s)
    assert L.dense_map_compare_frame(s, before=None)[0].tobytes() == h.compare(world, origins)[0].tobytes()
    assert L.dense_map_compare_frame(s, before=5, tolerance=0.4, max_range=20.0)[0].tobytes() == h.compare(world, origins, 0.4, 20.0, before=5)[0].tobytes()
    el = np.deg2rad(-15.0 + 2.0 * np.arange(16))
    T = np.asarray(s.world_transform(), np.float64).reshape(4, 4)
    scan = L.dense_map_render_scan(s, el, 360)
    o, t = L.scan_targets(T, el, 360)
    hh, hp = h.cast(o, t, extend=INF)
    assert scan.shape == (16, 360) and scan.tobytes() == hh.tobytes() and (scan["status"] == 1).sum() > 2000
    dh, dp = L.dense_map_cast(s, o, t, extend=INF)
    assert dh.tobytes() == hh.tobytes() and dp.tobytes() == hp.tobytes()
    assert L.dense_map_render_scan(s, el, 360, pose=T).tobytes() == scan.tobytes()
    s.close()


def test_a_box_that_is_in_no_earlier_frame_is_unmapped(L, drive):
    s, h, labels = pipeline(L, drive[:9], (8,), box_at=8)
    box = labels[8][-len(R.box_points()):]
    assert (box != 0).sum() > 30 and (box[box != 0] == 2).all()
    s.close()


def test_mode_2_on_a_non_keyframe_counts_every_voxel(L, drive):
    s = L.Slam(0, EgoMotion=3, DenseMap=2, DenseMapLeafSize=PIPE_LEAF)
    h = L.DenseMapHost(PIPE_LEAF)
    ordinal, kf, seen = 0, 0, set()
    for f, (pts, stamp) in enumerate(drive):
        s.add_frame(pts, stamp, f)
        now = int(s.stats()[13])
        world, origins = s.registered_frame().copy(), L.registered_frame_origins(s)
        inserted = now != kf
        if inserted:
            h.insert(world, ordinal)
        labels, counts = L.dense_map_compare_frame(s)
        hl, hc = h.compare(world, origins, before=ordinal if inserted else None)
        assert labels.tobytes() == hl.tobytes() and counts.tolist() == hc.tolist()
        ordinal += inserted
        kf = now
        seen.add(inserted)
    assert seen == {True, False}
    s.close()


def test_a_frame_that_did_not_go_into_the_map_is_compared_against_every_voxel(L, drive):
    """automatic `before` after a frame added while "DenseMap" was 0: the ordinal of the frame before must not be used"""
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF)
    h = L.DenseMapHost(PIPE_LEAF)
    for f in range(3):
        s.add_frame(*drive[f], f)
        h.insert(s.registered_frame(), f)
    s.set_param("DenseMap", 0)
    s.add_frame(*drive[3], 3)  # not inserted
    s.set_param("DenseMap", 1)
    world, origins = s.registered_frame().copy(), L.registered_frame_origins(s)
    labels, counts = L.dense_map_compare_frame(s)
    hl, hc = h.compare(world, origins)  # every voxel, those of ordinal 2 among them
    assert labels.tobytes() == hl.tobytes() and counts.tolist() == hc.tolist()
    assert labels.tobytes() != h.compare(world, origins, before=2)[0].tobytes()  # (the two answers differ on this drive)
    s.close()


def test_the_two_device_rig_is_labelled_in_registered_frame_order(L):
    leaf = 1.0
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=leaf)
    h = L.DenseMapHost(leaf)
    for f in range(3):
        frames, stamps, offset = two_device_rig(L, f)
        if f == 0:
            s.set_base_to_lidar_offset(offset, device_id=1)
            s.set_extractor_param(1, "EdgeIntensityGapThreshold", 40.0)
        s.add_frames(frames, stamps, f)
        world, origins = s.registered_frame().copy(), L.registered_frame_origins(s)
        assert world.size == frames[0].size + frames[1].size
        h.insert(world, f)
        labels, counts = L.dense_map_compare_frame(s)
        hl, hc = h.compare(world, origins, before=f)
        assert labels.tobytes() == hl.tobytes() and counts.tolist() == hc.tolist()
    assert (labels == 1).sum() > 100
    s.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(L, gpu_ctx):
    p = Pair(L, gpu_ctx)
    p.insert(K.ray_cloud(100), 0)
    lib, d = L.lib(), p.d
    o, t = np.zeros((1, 3), np.float32), R.xyz(K.ray_cloud(10))
    pts = K.ray_cloud(10)
    hits, points = np.full(10, 7, L.dense_hit_dtype), np.full(10, 7, L.POINT_DTYPE)
    labels, counts = np.full(10, 9, np.uint8), np.full(4, -5, np.int64)
    good = dict(max_range=30.0, extend=0.0, max_miss_ratio=-1.0, min_frames=1, use_before=0, before=0, reserved=0)

    def params(**change):
        q = L.DenseCastParams()
        for k, v in {**good, **change}.items():
            setattr(q, k, v)
        return C.byref(q)

    cast = lambda q=None, origins=o, n_origins=1, targets=t, n=10, out=hits: lib.lsa_dense_map_cast(  # noqa: E731
        d.h, L.ptr(origins) if origins is not None else None, n_origins, L.ptr(targets) if targets is not None else None, n, q, L.ptr(out) if out is not None else None, L.ptr(points))
    compare = lambda q=None, n=10, n_origins=1, out=labels: lib.lsa_dense_map_compare_points(  # noqa: E731
        d.h, L.ptr(pts), n, L.ptr(o), n_origins, q, L.ptr(out) if out is not None else None, L.ptr(counts))
    bad_params = [dict(max_range=v) for v in (0.0, -1.0, INF, float("nan"), 4096 * K.LEAF * 1.001)] + [dict(extend=float("nan")), dict(min_frames=0), dict(use_before=2),
                                                                                                         dict(use_before=-1), dict(reserved=1)]
    for change in bad_params:
        assert cast(params(**change)) == L.E_ARG and compare(params(**change)) == L.E_ARG, change
    for change in (dict(extend=-0.1), dict(extend=INF)):
        assert compare(params(**change)) == L.E_ARG and cast(params(**change)) == 0
    hits[:], points[:] = 7, 7
    assert cast(None) == L.E_ARG and cast(params(), origins=None) == L.E_ARG and cast(params(), targets=None) == L.E_ARG and cast(params(), out=None) == L.E_ARG
    assert cast(params(), n=-1) == L.E_ARG and cast(params(), n_origins=2) == L.E_ARG and cast(params(), n_origins=0) == L.E_ARG
    assert compare(None) == L.E_ARG and compare(params(), out=None) == L.E_ARG and compare(params(), n=-1) == L.E_ARG and compare(params(), n_origins=3) == L.E_ARG
    assert lib.lsa_dense_map_compare_points(d.h, L.ptr(pts), 10, L.ptr(o), 1, params(), L.ptr(labels), None) == L.E_ARG
    assert (hits == np.full(1, 7, L.dense_hit_dtype)).all() and (points == np.full(1, 7, L.POINT_DTYPE)).all() and (labels == 9).all() and (counts == -5).all()
    assert cast(params(), n=0) == 0 and compare(params(), n=0) == 0 and counts.tolist() == [0, 0, 0, 0] and (labels == 9).all()
    # the fused call: no frame's worth of room, a NULL pose
    gpu_ctx.upload_frame(L.synth_frame(16, 1000, 0)[0])
    n = lib.lsa_frame_size(gpu_ctx.h)
    big = np.full(n, 9, np.uint8)
    H = L.pose16(np.eye(4))
    assert lib.lsa_dense_map_compare_frame(d.h, 0, L.ptr(H), None, 0.0, 0.0, 0.0, params(), L.ptr(big), n - 1, L.ptr(counts)) == L.E_CAPACITY
    assert lib.lsa_dense_map_compare_frame(d.h, 0, None, None, 0.0, 0.0, 0.0, params(), L.ptr(big), n, L.ptr(counts)) == L.E_ARG
    assert lib.lsa_dense_map_compare_frame(d.h, 1, L.ptr(H), None, 0.0, 0.0, 0.0, params(), L.ptr(big), n, L.ptr(counts)) == L.E_ARG
    assert lib.lsa_dense_map_compare_frame(d.h, 0, L.ptr(H), None, 0.0, 0.0, 0.0, params(extend=-1.0), L.ptr(big), n, L.ptr(counts)) == L.E_ARG
    assert (big == 9).all() and counts.tolist() == [0, 0, 0, 0]
    assert lib.lsa_scan_targets(None, L.ptr(np.zeros(1)), 1, 1, L.ptr(np.zeros(3, np.float32)), L.ptr(np.zeros(3, np.float32))) == L.E_ARG
    K.same_state(p.d, p.h)
    assert d.get_param("CastRays") == 20 and d.get_param("CastSeconds") > 0  # the two casts that went through
    p.close()


def test_the_pipelines_calls_refuse_while_the_dense_map_is_off(L, drive):
    s = L.Slam(0, EgoMotion=3)
    s.add_frame(*drive[0], 0)
    o, t = np.zeros((1, 3), np.float32), np.ones((4, 3), np.float32)
    for call in (lambda: L.dense_map_cast(s, o, t), lambda: L.dense_map_render_scan(s, [0.0], 8), lambda: L.dense_map_compare_frame(s)):
        with pytest.raises(L.LsaError) as e:
            call()
        assert e.value.code == L.E_STATE
    s.set_param("DenseMap", 1)  # on, and no frame in it yet: an empty map answers
    hits, _ = L.dense_map_cast(s, o, t)
    assert (hits["status"] == 0).all() and (L.dense_map_compare_frame(s)[0] == 2).sum() > 1000
    with pytest.raises(L.LsaError) as e:
        L.dense_map_cast(s, o, t, max_range=-1.0)
    assert e.value.code == L.E_ARG
    s.close()
