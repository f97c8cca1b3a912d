"""Insertions of any size into the device maps: the second form of RollingGrid::Add's merge, whose scans of the chunk tables
live in global memory (lsa_grid_add.hip: k_scan_blocks / k_scan_addback / k_add_merge_global), against the oracle's
restatement of slam_lib/src/RollingGrid.cxx, byte for byte -- forced at small sizes around every seam of the scan
("GlobalScans"), and by its size alone for one Add of 3.3 million points: from host points, from a PCD file, from the
keypoint log, and through Slam.set_trajectory.  No tolerance is involved except where a registration follows.

What the oracle costs decides the shapes.  Its Add is a hash insertion per point (10 s for 3.3 M points into 3 M voxels) --
and for CENTROID sampling a loop over every voxel the Add has touched so far PER POINT (RollingGrid.cxx:282-297): a CENTROID
cloud of n points over V voxels costs n * V there, so the CENTROID clouds are narrow (many points, few voxels)."""
import time

import numpy as np
import pytest

import lidarslam_amd as L
from oracle import oracle as O
from test_gpu_device_grid import same_state, same_submap
from test_gpu_trajectory_correction import bend, box_of, expected_replay, rot
from test_rolling_grid import cloud

pytestmark = pytest.mark.gpu

GRID = dict(GridSize=50, VoxelResolution=10.0, LeafSize=0.6)
LEAF = 0.6


@pytest.fixture(scope="module")
def ctx():
    c = L.Context(0)
    yield c
    c.close()


def lattice(rng, v, t=0.0):
    """v points in v different leaf voxels: a lattice of the leaf size, 640 columns along x (-192 m .. 192 m), as many rows
    along y as it takes -- inside a grid of 50 voxels of 10 m around the origin"""
    i = np.arange(v)
    p = np.zeros(v, L.POINT_DTYPE)
    p["x"] = ((i % 640 - 320) * LEAF).astype(np.float32)
    p["y"] = ((i // 640 - (v // 640) // 2) * LEAF).astype(np.float32)
    p["z"] = 0.0
    p["intensity"] = rng.integers(0, 255, v).astype(np.float32)
    p["time"] = t
    return p[rng.permutation(v)]


def box(q):
    return (np.array([q["x"].min(), q["y"].min(), q["z"].min()], np.float32), np.array([q["x"].max(), q["y"].max(), q["z"].max()], np.float32))


class Trio:
    """the same calls on a device grid in the global form, one in the form its size picks (LDS at these sizes) and the oracle"""

    def __init__(self, ctx, form, ordered=1, **params):
        self.g, self.lds, self.o = L.DeviceGrid(ctx), L.DeviceGrid(ctx), O.RollingGrid(Ordered=ordered, **params)
        for d in (self.g, self.lds):
            d.set("Ordered", ordered)  # before the first insertion: exact from then on
            for k, v in params.items():
                d.set(k, v)
        self.g.set("GlobalScans", form)
        assert self.g.get_param("GlobalScans") == form and self.lds.get_param("GlobalScans") == 0

    def add(self, pts, **kw):
        for m in (self.g, self.lds, self.o):
            m.add(pts, **kw)

    def check(self, sub):
        """map, clean map, size and one sub-map: the oracle's; the other form: the same bytes"""
        same_state(self.g, self.o)
        mn, mx = sub
        same_submap(self.g, self.o, mn, mx, min_nb=100)
        assert self.lds.size() == self.g.size()
        for clean in (False, True):
            assert self.lds.get(clean=clean).tobytes() == self.g.get(clean=clean).tobytes()

    def close(self):
        self.g.close(), self.lds.close()


def spread_of(sampling, wide):
    """CENTROID: a narrow cloud (a thousand voxels or two), see the head of the file"""
    return wide if sampling != 4 else 1.5


CASES = [(s, o, m) for s in (2, 4) for o in (1, 0) for m in (0, 3)]  # MAX_INTENSITY / CENTROID, "Ordered", MinFramesPerVoxel


# ---- 1. both forms at the seams of the scan ------------------------------------------------------------------------------
# 256 entries per scan block: the table of the new voxels (an entry per 256 places of the sorted batch) ends a block at 256
# entries = 65 536 points; the second level would end at 256 * 65 536 points, out of a test's reach (test 1c reaches it with
# blocks of 64 entries).  The flags of CENTROID are scanned with an entry per POINT: one block at 256 points, two levels up to
# 65 536, three at 65 537.
@pytest.mark.parametrize("sampling,ordered,min_frames", CASES)
def test_the_seams_of_the_new_voxels_table(ctx, sampling, ordered, min_frames):
    rng = np.random.default_rng(500 + sampling * 8 + ordered * 2 + min_frames)
    t = Trio(ctx, 1, ordered, Sampling=sampling, MinFramesPerVoxel=min_frames, **GRID)
    for step, n in enumerate((1, 255, 256, 257, 65535, 65536, 65537, 257, 65537)):
        # into an empty map first, then into what the steps before left; every third step the centre moves on by 300 m and
        # the grid (250 m either way) after it, so that old voxels drop -- at once when the cloud is wide, two moves later
        # when it is narrow; the steps between stay where they are (frame counts rise); step 3 does not roll and sees
        # most or all of its points fall outside
        centre = np.array([100.0 * (step - step % 3), 0.0, 0.0])
        pts = cloud(rng, n, centre, spread=spread_of(sampling, 60.0), t=step * 0.1, labels=True)
        t.add(pts, time=step * 0.1, roll=(step % 4 != 3), fixed=(step == 5))
        t.check(box(cloud(rng, 200, centre, spread=20.0)))
    assert t.o.size() > 1000
    t.close()


# The table of the old voxels has an entry per 1024 voxels: a chunk ends at 1024 voxels, a scan block at 256 * 1024 = 262 144.
@pytest.mark.parametrize("voxels", [1023, 1024, 1025, 262143, 262144, 262145])
@pytest.mark.parametrize("sampling,ordered,min_frames", [(2, 1, 0), (4, 0, 3)])
def test_the_seams_of_the_survivors_table(ctx, voxels, sampling, ordered, min_frames):
    rng = np.random.default_rng(voxels + sampling)
    for roll in (False, True):
        t = Trio(ctx, 1, ordered, Sampling=sampling, MinFramesPerVoxel=min_frames, **GRID)
        t.add(lattice(rng, voxels), roll=False)
        assert t.o.size() == voxels == t.g.size()  # (and the device grid's bound on its voxels is the number itself now)
        # 257 points 300 m down the x axis: the grid follows them by about ten voxels and the lattice's far end drops
        pts = cloud(rng, 257, np.array([300.0, 0.0, 0.0]), spread=10.0, t=0.1)
        t.add(pts, time=0.1, roll=roll)
        t.check((np.array([-120.0, -5.0, -1.0], np.float32), np.array([150.0, 5.0, 1.0], np.float32)))
        got = t.o.get()
        old = int((got["x"] < 200.0).sum())  # (the lattice ends at 192 m, the cloud begins beyond 250 m)
        if roll:
            assert got["x"].min() > -190.0 and 0.8 * voxels < old < voxels and got.size > old  # some dropped, most survive
        else:
            assert got.size == old == voxels  # nothing dropped, and the points fell outside the grid
        # once more where the grid stands now: every old voxel survives, new ones between them
        pts = cloud(rng, 257, np.array([100.0, 0.0, 0.0]), spread=10.0, t=0.2)
        t.add(pts, time=0.2, roll=False)
        t.check((np.array([60.0, -30.0, -5.0], np.float32), np.array([140.0, 30.0, 5.0], np.float32)))
        t.close()


# Scan blocks of 64 entries ("GlobalScans" = 2): a level ends at 64 entries = 16 384 points, the second one at 4096 entries
# = 1 048 576 points, where a third level begins; on the survivors' side at 64 chunks = 65 536 voxels.
@pytest.mark.parametrize("n,voxels", [(16383, 65535), (16384, 65536), (16385, 65537), (1048575, 65535), (1048576, 65536), (1048577, 65537)])
def test_the_second_level_of_the_scan_ends_too(ctx, n, voxels):
    rng = np.random.default_rng(n)
    t = Trio(ctx, 2, 1, Sampling=2, **GRID)
    t.add(lattice(rng, voxels), roll=False)
    assert t.o.size() == voxels == t.g.size()
    pts = cloud(rng, n, np.array([120.0, 0.0, 0.0]), spread=60.0, t=0.1)
    t.add(pts, time=0.1)
    t.check(box(cloud(rng, 200, np.array([120.0, 0.0, 0.0]), spread=20.0)))
    assert voxels // 2 < t.o.get().size  # (most of the lattice is still there)
    t.close()


def test_the_knob_is_one_of_three_values(ctx):
    g = L.DeviceGrid(ctx)
    for bad in (-1, 3, 0.5):
        with pytest.raises(L.LsaError):
            g.set("GlobalScans", bad)
    g.close()


# ---- 2. one insertion above the old limit, the form chosen by its size ----------------------------------------------------
BIG = 3300000  # 12 891 entries for the batch alone: more than the 12 288 that fit LDS


def big_case(sampling):
    """a map of a few hundred thousand voxels (100 Adds of 3000 points: the oracle's CENTROID loop again) and the cloud"""
    rng = np.random.default_rng(3300 + sampling)
    base = [cloud(rng, 3000, np.zeros(3), spread=60.0, t=0.0) for _ in range(100)]
    pts = cloud(rng, BIG, np.array([30.0, 0.0, 0.0]), spread=70.0 if sampling != 4 else 0.5, t=0.1)
    pts["w"] = 1.0  # (what a PCD file, which has no such field, gives back)
    o = O.RollingGrid(Sampling=sampling, **GRID)
    t0 = time.perf_counter()
    for b in base:
        o.add(b, roll=False)
    assert o.size() > 200000
    o.add(pts, time=0.1)
    print(f"oracle, sampling {sampling}: {time.perf_counter() - t0:.1f} s for the base and {BIG} points")
    return base, pts, o


@pytest.fixture(scope="module")
def big_max_intensity():
    """computed once, shared by the host-points test and the file test, left as it is"""
    return big_case(2)


def device_base(ctx, base, sampling):
    g = L.DeviceGrid(ctx, Sampling=sampling, **GRID)
    for b in base:
        g.add(b, roll=False)
    return g


SUB = (np.array([-20.0, -40.0, -5.0], np.float32), np.array([80.0, 40.0, 5.0], np.float32))


@pytest.mark.parametrize("sampling", [2, 4])
def test_one_insertion_above_the_old_limit(ctx, big_max_intensity, sampling):
    base, pts, o = big_max_intensity if sampling == 2 else big_case(4)
    g = device_base(ctx, base, sampling)
    g.add(pts, time=0.1)  # LSA_E_CAPACITY before the scans left LDS
    assert g.size() == o.size()
    assert g.get_param("Voxels") == o.get().size
    assert g.get().tobytes() == o.get().tobytes()
    assert same_submap(g, o, *SUB, min_nb=100) > 1000
    g.close()


# ---- 3. the same through a file -------------------------------------------------------------------------------------------
def test_a_prior_map_above_the_old_limit_from_a_file(ctx, big_max_intensity, tmp_path):
    base, pts, o = big_max_intensity
    path = tmp_path / "planes.pcd"
    assert L.write_pcd(path, pts, L.PCD_BINARY)
    g = device_base(ctx, base, 2)
    g.add_pcd(path, time=0.1)
    assert g.size() == o.size()
    assert g.get().tobytes() == o.get().tobytes()
    g.close()


# ---- 4. the log ------------------------------------------------------------------------------------------------------------
def test_a_long_log_is_replayed_into_device_maps(ctx):
    """42 frames of 80 000 planes (3.36 M) and 1000 edges under a bent trajectory: lsa_kplog_replay_to_grids, then the roll onto
    the last frame's box -- Slam.cxx:426-477 from oracle primitives, as test_rebuilt_maps_are_the_references states it"""
    rng = np.random.default_rng(42)
    frames, per = 42, 80000

    def pts(n):
        p = np.zeros(n, L.POINT_DTYPE)
        p["x"], p["y"], p["z"] = (rng.uniform(-s, s, n).astype(np.float32) for s in (60, 60, 3))
        p["w"] = 1.0
        p["time"] = rng.uniform(-0.1, 0.0, n)
        p["intensity"] = rng.uniform(0, 255, n).astype(np.float32)
        p["laser_id"] = rng.integers(0, 128, n)
        return p

    log = [[pts(1000), pts(per), pts(0)] for _ in range(frames)]
    P = [np.eye(4)]
    for _ in range(frames - 1):
        D = np.eye(4)
        D[:3, :3] = rot([0.1, 0.2, 1.0], rng.uniform(0.0, 0.02))
        D[:3, 3] = [1.0, rng.uniform(-0.1, 0.1), 0.0]
        P.append(P[-1] @ D)
    P2 = bend(np.array(P))
    t = 100.0 + 0.1 * np.arange(frames)
    leaves = {L.EDGE: 0.3, L.PLANE: 0.6}
    grids = [L.DeviceGrid(ctx, GridSize=50, VoxelResolution=10.0, LeafSize=leaves[k]) for k in (L.EDGE, L.PLANE)]
    ctx.kplog_clear()
    try:
        for fr in log:
            ctx.kplog_append_points(fr)
        assert sum(ctx.kplog_count(i, L.PLANE) for i in range(frames)) == frames * per > 3200000
        mn, mx = ctx.kplog_replay_to_grids(P2, t, grids + [None], undistort=True)
    finally:
        ctx.kplog_clear()
    for k in (L.EDGE, L.PLANE):
        exp = expected_replay(O, [fr[k] for fr in log], P2, t, True)
        o = O.RollingGrid(GridSize=50, VoxelResolution=10.0, LeafSize=leaves[k])
        o.add(np.concatenate(exp), fixed=False, time=-1.0, roll=False)
        lo, hi = box_of(exp[-1])
        assert mn[k].tobytes() == lo.tobytes() and mx[k].tobytes() == hi.tobytes()
        o.roll(lo, hi)
        grids[k].roll(mn[k], mx[k])
        want, got = o.get(), grids[k].get()
        assert got.size == want.size > 500, (k, got.size, want.size)
        assert got.tobytes() == want.tobytes(), k
        grids[k].close()


# ---- 5. the public call ---------------------------------------------------------------------------------------------------
def test_a_long_session_is_rebuilt_on_the_device(ctx):
    """128 rings until more than 3 000 000 planes are logged (the refusal's old threshold): set_trajectory is accepted with
    the maps on the device, and leaves the maps the host-map route leaves (which is held to the oracle in
    test_gpu_trajectory_correction.py); both go on with the next frame"""
    t0 = time.perf_counter()
    dev = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, MapsOnDevice=1)
    host = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, MapsOnDevice=0)
    planes, f = 0, 0
    while planes <= 3000000:
        pts, stamp = L.synth_frame(128, 1000, f)
        for s in (dev, host):
            s.add_frame(pts, stamp, f)
        assert dev.logged_frames() == f + 1
        planes += dev.context().kplog_count(f, L.PLANE)
        f += 1
    assert planes == sum(host.context().kplog_count(i, L.PLANE) for i in range(f))
    n = f
    ends = {}
    for name, s in (("device", dev), ("host", host)):
        P, t, _ = s.trajectory()
        assert P.shape[0] == n == s.logged_frames()
        P2 = bend(P)
        s.set_trajectory(P2, t)  # the device maps: LSA_E_CAPACITY before
        ends[name] = (P2, t)
    for k in (L.EDGE, L.PLANE):
        a, b = dev.map(k), host.map(k)
        assert a.size == b.size > 1000, (k, a.size, b.size)
        assert a.tobytes() == b.tobytes(), k
    # life goes on, on both: the next frame is registered in the rebuilt map
    pts, stamp = L.synth_frame(128, 1000, n)
    counts = {}
    for name, s in (("device", dev), ("host", host)):
        s.add_frame(pts, stamp, n)
        counts[name] = [s.keypoints(k, which=2).size for k in (L.EDGE, L.PLANE)]
        Pn, _, _ = s.trajectory()
        P2 = ends[name][0]
        assert Pn.shape[0] == n + 1 and Pn[:n].tobytes() == P2.tobytes()
        assert np.all(np.isfinite(Pn))
        # (the bound of test_life_goes_on_after_a_rebuild: on from the bent trajectory's end, within a metre)
        assert np.linalg.norm(Pn[n][:3, 3] - P2[-1][:3, 3]) < 1.0
        ends[name] = Pn[n]
    assert counts["device"] == counts["host"] and min(counts["device"]) > 100
    assert np.linalg.norm(ends["device"][:3, 3] - ends["host"][:3, 3]) < 1.0
    dev.close(), host.close()
    print(f"the public call: {n} frames, {planes} planes, {time.perf_counter() - t0:.1f} s")
