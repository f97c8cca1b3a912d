"""Place recognition against the maps: k_map_slice_boxes / k_map_describe / k_map_finish, the context's table of map
descriptors, k_place_search on it, and recognize_place_in_maps on top of them.

The reference is the host statement (L.map_descriptor, L.scan_descriptor, L.place_distance, L.map_place_select), which compiles
the same definition (lidarslam_amd/csrc/lsa_scan_descriptor.h) and which tests/test_map_place_host.py and
tests/test_place_host.py hold to numpy: device and host must agree byte for byte -- cells, norms, distances, shifts, candidates."""
import math
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example

pytestmark = pytest.mark.gpu

# rings, sectors, the other parameters
SHAPES = [
    (1, 1, {}),
    (3, 7, dict(min_range=2.5, max_range=50.0, height_offset=1.25)),
    (20, 60, {}),
    (32, 120, dict(height_offset=-1.0)),
]
SLICE = 64  # "map_describe_slice" of the sliced runs: 5 000 points are 79 slices
MARGIN = 1.0 + 2.0 ** -20


def points(L, xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(xyz.shape[0], L.POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    return p


def xyz_of(pts):
    return np.column_stack([pts["x"], pts["y"], pts["z"]])


def special_slices(rng):
    """Five slices of SLICE points each, seen from the viewpoint at the origin: one contended cell; NaNs; points exactly on the
    ring borders of every shape; points on the sector borders; points 1e-4 m on either side of both max_range (50 and 80)."""
    one_cell = np.column_stack([10.0 + rng.uniform(0, 0.01, SLICE), 10.0 + rng.uniform(0, 0.01, SLICE), rng.uniform(-5, 5, SLICE)])
    nan = np.column_stack([rng.uniform(-40, 40, SLICE), rng.uniform(-40, 40, SLICE), rng.uniform(-4, 6, SLICE)])
    nan[0::4, 0] = np.nan
    nan[1::4, 1] = np.nan
    nan[2::4, 2] = np.nan
    rings = []
    for n, _, extra in SHAPES:
        lo, hi = extra.get("min_range", 0.0), extra.get("max_range", 80.0)
        for k in range(n + 1):
            r = np.float32(k * (hi - lo) / n + lo)
            rings += [(r, 0.0), (-r, 0.0), (0.0, r), (0.0, -r)]
    rings = np.array(rings, np.float64)[rng.permutation(len(rings))[:SLICE]]
    rings = np.column_stack([rings, rng.uniform(-3, 3, SLICE)])
    sectors = []
    for _, n, _ in SHAPES:
        for k in range(n):
            a = -np.pi + k * 2 * np.pi / n
            sectors.append((7.5 * np.cos(a), 7.5 * np.sin(a)))
    sectors = np.array(sectors)[rng.permutation(len(sectors))[:SLICE]]
    sectors = np.column_stack([sectors, rng.uniform(-3, 3, SLICE)])
    edge = []
    for hi in (50.0, 80.0):
        for k in range(SLICE // 4):
            a = rng.uniform(-np.pi, np.pi)
            for r in (hi - 1e-4, hi + 1e-4):
                edge.append((r * np.cos(a), r * np.sin(a), rng.uniform(0, 3)))
    return np.vstack([one_cell, nan, rings, sectors, np.array(edge)]).astype(np.float32)


@pytest.fixture(scope="module")
def strip(L):
    """5 000 map points: the special slices, then a strip 600 m long sorted by x, so that a slice is spatially compact (as the
    key-sorted array of a device grid is); 65 viewpoints: the origin, one beside it, one 1e5 m away, the rest along the strip"""
    rng = np.random.default_rng(20261020)
    special = special_slices(rng)
    n = 5000 - special.shape[0]
    cloud = np.column_stack([np.sort(rng.uniform(-300, 300, n)), rng.uniform(-40, 40, n), rng.uniform(-4, 6, n)]).astype(np.float32)
    pts = points(L, np.vstack([special, cloud]))
    assert pts.size == 5000
    vp = np.zeros((65, 3))
    vp[1] = [12.5, -7.25, 0.5]
    vp[2] = [1e5, 0.0, 0.0]
    vp[3:, 0] = np.linspace(-310, 310, 62)
    vp[3:, 1] = rng.uniform(-20, 20, 62)
    vp[3:, 2] = rng.uniform(-1, 1, 62)
    return pts, vp


def np_boxes(pts, slice_size):
    out = []
    for b in range(0, pts.size, slice_size):
        x, y = pts["x"][b:b + slice_size], pts["y"][b:b + slice_size]
        x, y = x[~np.isnan(x)], y[~np.isnan(y)]
        out.append([x.min() if x.size else np.finfo(np.float32).max, y.min() if y.size else np.finfo(np.float32).max,
                    x.max() if x.size else -np.finfo(np.float32).max, y.max() if y.size else -np.finfo(np.float32).max])
    return np.array(out, np.float32).reshape(-1, 4)


def out_of_reach(boxes, vp, max_range):
    """(V, slices): the planar distance from the viewpoint to the slice's box exceeds max_range * (1 + 2^-20)"""
    b = boxes.astype(np.float64)
    dx = np.maximum(np.maximum(b[None, :, 0] - vp[:, None, 0], vp[:, None, 0] - b[None, :, 2]), 0.0)
    dy = np.maximum(np.maximum(b[None, :, 1] - vp[:, None, 1], vp[:, None, 1] - b[None, :, 3]), 0.0)
    return dx * dx + dy * dy > (max_range * MARGIN) ** 2


@pytest.mark.parametrize("rings,sectors,extra", SHAPES)
def test_descriptors_equal_the_host_statement(L, gpu_ctx, strip, rings, sectors, extra):
    ctx = gpu_ctx
    pts, vp = strip
    p = dict(rings=rings, sectors=sectors, **extra)
    length = rings * sectors + sectors
    occupied, passed_over, in_reach = 0, 0, 0
    try:
        for n, slice_size in [(0, 0), (1, 0), (255, 0), (256, 0), (257, 0), (257, SLICE), (5000, SLICE), (5000, 0)]:
            want = np.array([L.map_descriptor(pts[:n], v, **p) for v in vp]).reshape(len(vp), length)
            for V in (1, 2, 65):
                got = {}
                for cull in (1, 0):
                    ctx.debug_set("map_describe_slice", slice_size)
                    ctx.debug_set("map_describe_cull", cull)
                    assert L.map_place_describe(ctx, pts[:n], vp[:V], **p) == V
                    got[cull] = L.map_place_descriptors(ctx, 0, V - 1, **p)
                    boxes = L.map_place_slices(ctx)
                    assert boxes.shape[0] == -(-n // (slice_size or 4096))
                    assert boxes.tobytes() == np_boxes(pts[:n], slice_size or 4096).tobytes()
                assert got[1].tobytes() == got[0].tobytes(), (rings, sectors, n, slice_size, V)
                assert got[1].tobytes() == want[:V].tobytes(), (rings, sectors, n, slice_size, V, np.argwhere(got[1].view(np.uint32) != want[:V].view(np.uint32))[:8])
                far = out_of_reach(boxes, vp[:V], extra.get("max_range", 80.0))
                passed_over += int(far.sum())
                in_reach += int((~far).sum())
            occupied += int((want > 0).sum())
            if n == 5000:
                assert not want[2].any()  # 1e5 m away: out of reach of everything
    finally:
        ctx.debug_set("map_describe_slice", 0)
        ctx.debug_set("map_describe_cull", 1)
    print("shape", (rings, sectors), "occupied cells", occupied, "(viewpoint, slice) pairs passed over", passed_over, "in reach", in_reach)
    assert occupied > 0 and passed_over > 0 and in_reach > 0


def test_special_slices_are_what_they_claim(L, strip):
    """on the host statement: seen from the origin the contended slice fills one cell, and of the points 1e-4 m on either side
    of max_range exactly the inner half takes part"""
    pts, _ = strip
    d = L.map_descriptor(pts[:SLICE], [0, 0, 0])
    assert np.count_nonzero(d[:1200]) == 1 and d[:1200].max() == np.float32(pts["z"][:SLICE].max() + np.float32(2.0))
    edge = pts[4 * SLICE:5 * SLICE]
    r = np.hypot(edge["x"].astype(np.float64), edge["y"].astype(np.float64))
    assert np.all(np.abs(np.abs(r - 65.0) - 15.0) < 2e-4) and ((r < 80.0) & (r > 70.0)).sum() == SLICE // 4 and (r < 50.0).sum() == SLICE // 4
    inner = L.map_descriptor(edge[(r < 80.0) & (r > 70.0)], [0, 0, 0], rings=1, sectors=1)
    assert inner[0] > 0 and not L.map_descriptor(edge[r >= 80.0], [0, 0, 0], rings=1, sectors=1).any()


# ---- grids as the source -------------------------------------------------------------------------------------------------------
def test_grids_as_the_source(L, gpu_ctx):
    ctx = gpu_ctx
    rng = np.random.default_rng(7)
    grids = [L.DeviceGrid(ctx) for _ in range(3)]
    vp = np.array([[0.0, 0.0, 0.0], [30.0, 5.0, 0.5], [62.0, -3.0, 0.2], [1e4, 0.0, 0.0]])
    try:
        def cloud(n, x0):
            return points(L, np.column_stack([x0 + rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(-3, 6, n)]))

        for k, g in enumerate(grids):  # two batches with a roll between: the second moves the grid
            g.add(cloud(3000 + 500 * k, 0.0), time=1.0)
            g.add(cloud(2000, 150.0), time=2.0)
        held = [g.get() for g in grids]
        assert all(h.size > 1000 for h in held) and len({h.size for h in held}) == 3
        ctx.debug_set("map_describe_slice", 256)
        for rings, sectors, extra in SHAPES[1:]:
            for mask in range(1, 8):
                p = dict(rings=rings, sectors=sectors, type_mask=mask, **extra)
                assert L.map_place_describe(ctx, grids, vp, **p) == len(vp)  # the parameters changed: everything again
                got = L.map_place_descriptors(ctx, 0, len(vp) - 1, **p)
                src = np.concatenate([held[k] for k in range(3) if (mask >> k) & 1])
                want = np.array([L.map_descriptor(src, v, **p) for v in vp])
                assert got.tobytes() == want.tobytes(), (rings, sectors, mask)
                assert want[:3].any() and not want[3].any()
        # a grid that is not given takes no part, whatever the mask says
        p = dict(rings=20, sectors=60, type_mask=7)
        assert L.map_place_describe(ctx, [grids[0], None, grids[2]], vp, **p) == len(vp)
        want = np.array([L.map_descriptor(np.concatenate([held[0], held[2]]), v, **p) for v in vp])
        assert L.map_place_descriptors(ctx, 0, len(vp) - 1, **p).tobytes() == want.tobytes()
        # the table is kept while nothing changes, and made again when a map, the viewpoints or the parameters do
        p = dict(rings=20, sectors=60, type_mask=3)
        assert L.map_place_describe(ctx, grids, vp, **p) == len(vp)
        assert L.map_place_describe(ctx, grids, vp, **p) == 0
        assert grids[0].size() > 0 and grids[1].get().size == held[1].size  # calls that change nothing
        assert L.map_place_describe(ctx, grids, vp.copy(), **p) == 0       # the viewpoints are compared by content
        grids[2].add(cloud(100, 0.0), time=3.0)                            # a map outside the mask
        assert L.map_place_describe(ctx, grids, vp, **p) == 0
        grids[1].add(cloud(700, 20.0), time=3.0)
        assert L.map_place_describe(ctx, grids, vp, **p) == len(vp)
        src = np.concatenate([grids[0].get(), grids[1].get()])
        want = np.array([L.map_descriptor(src, v, **p) for v in vp])
        assert L.map_place_descriptors(ctx, 0, len(vp) - 1, **p).tobytes() == want.tobytes()
        assert L.map_place_describe(ctx, grids, vp, **p) == 0
        moved = vp.copy()
        moved[1, 0] += 1e-9
        assert L.map_place_describe(ctx, grids, moved, **p) == len(vp)
        assert L.map_place_describe(ctx, grids, moved, **dict(p, height_offset=2.5)) == len(vp)
        assert L.map_place_describe(ctx, grids, moved[:2], **dict(p, height_offset=2.5)) == 2
        grids[0].clear()
        grids[1].clear()
        assert L.map_place_describe(ctx, grids, vp, **p) == len(vp)  # empty maps describe to zeros
        assert not L.map_place_descriptors(ctx, 0, len(vp) - 1, **p).any()
    finally:
        ctx.debug_set("map_describe_slice", 0)
        for g in grids:
            g.close()


# ---- the search ----------------------------------------------------------------------------------------------------------------
def island_cloud(rng, kind, sectors_of_pattern=60):
    """a cloud around the origin on a grid of 1/256 m (exact wherever an island is put): random, or the same column of points in
    every third sector (ties between shifts)"""
    if kind == "random":
        xyz = np.column_stack([rng.uniform(-60, 60, 400), rng.uniform(-60, 60, 400), rng.uniform(-1, 6, 400)])
    else:
        offset = {"periodic": 0, "periodic+2": 2}[kind]
        r = np.array([5.0, 17.0, 29.0, 41.0, 53.0])
        z = np.array([0.5, 3.0, 1.25, 4.0, 2.0])
        a = -np.pi + (np.arange(offset, sectors_of_pattern, 3) + 0.5) * 2 * np.pi / sectors_of_pattern
        xyz = np.column_stack([np.outer(np.cos(a), r).ravel(), np.outer(np.sin(a), r).ravel(), np.tile(z, a.size)])
    return np.round(xyz * 256) / 256


@pytest.mark.parametrize("V", [1, 2, 65, 300])
def test_search_equals_the_host_statement(L, gpu_ctx, V):
    """Islands 256 m apart on a square grid, a viewpoint in the middle of each: empty, the query's cloud itself, the query's
    cloud a quarter turned, periodic clouds, random ones.  Both launch shapes of k_place_search."""
    ctx = gpu_ctx
    rng = np.random.default_rng(100 + V)
    query = {"random": island_cloud(rng, "random"), "periodic": island_cloud(rng, "periodic")}
    side = int(np.ceil(np.sqrt(V)))
    vp = np.array([[256.0 * (i % side), 256.0 * (i // side), 0.0] for i in range(V)])
    kinds = ["same", "empty", "turned", "periodic", "periodic+2", "other"]
    islands, kind_of = [], []
    for i in range(V):
        kind = kinds[i % len(kinds)] if V > 1 else "same"
        kind_of.append(kind)
        if kind == "empty":
            continue
        base = {"same": query["random"], "turned": query["random"] @ np.array([[0.0, 1.0, 0], [-1.0, 0, 0], [0, 0, 1.0]]), "other": island_cloud(rng, "random")}.get(kind)
        if base is None:
            base = island_cloud(rng, kind)
        islands.append(base + vp[i])
    pts = points(L, np.vstack(islands))
    assert np.array_equal(xyz_of(pts).astype(np.float64), np.vstack(islands))  # the grid of 1/256 m is exact in float32
    order = np.argsort(pts["x"], kind="stable")
    pts = pts[order]
    try:
        for rings, sectors, extra in SHAPES[1:]:
            p = dict(rings=rings, sectors=sectors, **extra)
            ctx.debug_set("map_describe_slice", 128)
            assert L.map_place_describe(ctx, pts, vp, **p) == V
            table = [L.map_descriptor(pts, v, **p) for v in vp]
            for name, cloud in query.items():
                frame = [points(L, cloud[k::3]) for k in range(3)]
                for mask in (5, 7):
                    q = dict(p, type_mask=mask)
                    # (the mask is the query's: the table holds whatever points it was given)
                    assert L.map_place_describe(ctx, pts, vp, **q) == V
                    for k in range(3):
                        ctx.set_keypoints(L.SET_WORKING, k, frame[k])
                    dq = L.scan_descriptor(np.concatenate([frame[k] for k in range(3) if (mask >> k) & 1]), **q)
                    want = [L.place_distance(dq, d, **q) for d in table]
                    for blocks in (0, 3):
                        ctx.debug_set("place_max_blocks", blocks)
                        dist, shift = L.map_place_search(ctx, L.SET_WORKING, **q)
                        assert dist.dtype == np.float32 and shift.dtype == np.int32 and dist.size == shift.size == V
                        assert [(d, int(s)) for d, s in zip(dist, shift)] == want, (V, rings, sectors, name, mask, blocks)
                        assert L.map_place_descriptors(ctx, V, V, **q)[0].tobytes() == dq.tobytes()  # the query's slot
                    if name == "random" and mask == 7 and sectors % 4 == 0:
                        for i, kind in enumerate(kind_of):
                            if kind == "same":
                                assert want[i][1] == 0 and want[i][0] < 1e-6
                            if kind == "turned":
                                assert want[i][1] == sectors // 4 and want[i][0] < 0.05
                            if kind == "empty":
                                assert want[i] == (np.float32(1.0), 0)
                    if name == "periodic" and mask == 7 and sectors == 60:
                        for i, kind in enumerate(kind_of):
                            if kind == "periodic":
                                assert want[i][1] == 0 and want[i][0] < 1e-6
                            if kind == "periodic+2":
                                assert want[i][1] == 2 and want[i][0] < 1e-6
    finally:
        ctx.debug_set("place_max_blocks", 0)
        ctx.debug_set("map_describe_slice", 0)
        for k in range(3):
            ctx.set_keypoints(L.SET_WORKING, k, points(L, np.zeros((0, 3))))


# ---- refusals write nothing ------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(L):
    ctx = L.Context(0)
    other = L.Context(0)
    try:
        pts = points(L, np.random.default_rng(3).uniform(-30, 30, (500, 3)))
        vp = np.array([[0.0, 0.0, 0.0], [5.0, 5.0, 0.0]])
        p = dict(rings=20, sectors=60)
        dist, shift = np.full(4, 7.0, np.float32), np.full(4, -7, np.int32)
        out = np.full((3, 1260), -1.0, np.float32)

        def refused(code, call):
            with pytest.raises(L.LsaError) as e:
                call()
            assert e.value.code == code, str(e.value)
            assert np.all(dist == 7.0) and np.all(shift == -7) and np.all(out == -1.0)

        # no table yet
        refused(L.E_STATE, lambda: L.map_place_search(ctx, L.SET_WORKING, out=(dist, shift), **p))
        refused(L.E_STATE, lambda: L.map_place_descriptors(ctx, 0, 0, out=out, **p))
        refused(L.E_STATE, lambda: L.map_place_slices(ctx))
        for bad in (dict(rings=0), dict(sectors=121), dict(type_mask=0), dict(max_range=-1.0), dict(height_offset=float("inf"))):
            refused(L.E_ARG, lambda: L.map_place_describe(ctx, pts, vp, **bad))
        refused(L.E_ARG, lambda: L.map_place_describe(ctx, pts, vp[:0], **p))
        for v in (np.nan, np.inf, -np.inf):
            broken = vp.copy()
            broken[1, 2] = v
            refused(L.E_ARG, lambda: L.map_place_describe(ctx, pts, broken, **p))
        g = L.DeviceGrid(other)
        refused(L.E_ARG, lambda: L.map_place_describe(ctx, [g, None, None], vp, **p))
        g.close()
        assert ctx.L.lsa_map_place_viewpoints(ctx.h) == 0
        # a table, and the refusals that leave it as it is
        assert L.map_place_describe(ctx, pts, vp, **p) == 2
        table = L.map_place_descriptors(ctx, 0, 1, **p)
        assert table.any()
        refused(L.E_STATE, lambda: L.map_place_search(ctx, L.SET_WORKING, out=(dist, shift), **p))            # an empty query set
        ctx.set_keypoints(L.SET_WORKING, L.PLANE, pts[:50])
        refused(L.E_STATE, lambda: L.map_place_search(ctx, L.SET_WORKING, out=(dist, shift), **dict(p, type_mask=1)))  # ... of the mask's types
        refused(L.E_STATE, lambda: L.map_place_search(ctx, L.SET_WORKING, out=(dist, shift), **dict(p, type_mask=1, rings=21)))  # other parameters than the table's
        refused(L.E_ARG, lambda: L.map_place_search(ctx, 3, out=(dist, shift), **p))
        refused(L.E_ARG, lambda: L.map_place_search(ctx, L.SET_WORKING, out=(dist, shift), **dict(p, sectors=0)))
        refused(L.E_STATE, lambda: L.map_place_descriptors(ctx, 0, 2, out=out, **p))  # the query's slot before a search
        refused(L.E_ARG, lambda: L.map_place_descriptors(ctx, 0, 3, out=out, **p))
        refused(L.E_ARG, lambda: L.map_place_descriptors(ctx, 1, 0, out=out, **p))
        refused(L.E_ARG, lambda: L.map_place_describe(ctx, pts, vp, **dict(p, rings=33)))
        assert L.map_place_descriptors(ctx, 0, 1, **p).tobytes() == table.tobytes()
        d, s = L.map_place_search(ctx, L.SET_WORKING, **p)
        dq = L.scan_descriptor(pts[:50], **p)
        assert [(a, int(b)) for a, b in zip(d, s)] == [L.place_distance(dq, t, **p) for t in table]
        assert L.map_place_descriptors(ctx, 0, 2, **p)[2].tobytes() == dq.tobytes()
    finally:
        other.close()
        ctx.close()


# ---- two sessions: map, save; load, recognise, localize ---------------------------------------------------------------------------
MODEL, MAPPED, QUERY, AFTER = 16, 30, 17, 6
# The oracle analogue on the CPU (an oracle Slam maps frames 0..29 of seed 1000, MapUpdate = 0, frame 17 of seed 1001 turned by 90
# degrees, SetWorldTransformFromGuess, frames 18..23 turned alike; viewpoints at the 30 mapping positions): the recognised start is
# viewpoint 17 with shift 16, 0.0 m and 0.066 rad from the true pose; after +6 the session started from it is 0.0610 m and 0.00692 rad
# from the control session started from the true pose (0.104 m / 0.016 rad against 0.052 m / 0.011 rad from the mapping
# trajectory).  The bound is twice the control-to-recognised distance.
BOUND_M, BOUND_RAD = 2 * 0.0610, 2 * 0.00692


def turned(pts):
    """the cloud as the sensor sees it with the base turned by +90 degrees about z (exactly: x' = y, y' = -x)"""
    out = pts.copy()
    out["x"], out["y"] = pts["y"], -pts["x"]
    return out


def Rz(yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    return T


def pose_diff(ref, cur):
    D = np.linalg.inv(ref) @ cur
    return float(np.linalg.norm(D[:3, 3])), float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


@pytest.fixture(scope="module")
def mapped(L, tmp_path_factory):
    """session A: 30 frames of seed 1000 with the keypoint log on, the maps saved as PCD, the logged poses"""
    prefix = str(tmp_path_factory.mktemp("maps") / "a_")
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    for f in range(MAPPED):
        pts, stamp = L.synth_frame(MODEL, 1000, f)
        s.add_frame(pts, stamp, f)
    P, _, _ = s.trajectory()
    assert P.shape[0] == MAPPED
    counts = s.save_maps_pcd(prefix, filtered=False)
    assert counts[0] > 1000 and counts[1] > 1000
    s.close()
    return prefix, P


def session_b(L, prefix, **params):
    s = L.Slam(0, EgoMotion=3, MapUpdate=0, **params)
    s.load_maps_pcd(prefix)
    pts, stamp = L.synth_frame(MODEL, 1001, QUERY)
    s.add_frame(turned(pts), stamp, 0)
    return s


def go_on(L, s, guess):
    s.set_world_transform_from_guess(guess)
    for i, f in enumerate(range(QUERY + 1, QUERY + 1 + AFTER)):
        pts, stamp = L.synth_frame(MODEL, 1001, f)
        s.add_frame(turned(pts), stamp, 1 + i)
    return s.world_transform()


def host_recognize(L, s, vp, capacity, search, **descriptor):
    mask = descriptor.get("type_mask", 3)
    maps = np.concatenate([s.map(k) for k in range(3) if (mask >> k) & 1])
    query = L.scan_descriptor(np.concatenate([s.keypoints(k, which=2) for k in range(3) if (mask >> k) & 1]), **descriptor)
    table = [L.place_distance(query, L.map_descriptor(maps, v, **descriptor), **descriptor) for v in vp]
    return L.map_place_select([d for d, _ in table], [sh for _, sh in table], vp, capacity=capacity, **search, **descriptor)


def same_candidates(got, want):
    return len(got) == len(want) and all(a[:4] == b[:4] and np.array_equal(a[4], b[4]) for a, b in zip(got, want))


@pytest.mark.parametrize("on_device", [1, 0])
def test_relocalization_in_a_loaded_map(L, mapped, on_device):
    prefix, P = mapped
    vp = P[:, :3, 3].copy()
    true = P[QUERY] @ Rz(np.pi / 2)
    b = session_b(L, prefix, MapsOnDevice=on_device)
    # the call against the host statement on what the session holds, exactly
    for search, descriptor in [
        (dict(), {}),
        (dict(exclusion_radius=1.2, max_descriptor_distance=0.25), dict(rings=32, sectors=120, type_mask=7)),
        (dict(exclusion_radius=0.0, max_distance=4.0, near_xyz=tuple(vp[20])), dict(rings=3, sectors=7, min_range=2.5, max_range=50.0, type_mask=2)),
    ]:
        for capacity in (0, 1, 4):
            got, summary = L.recognize_place_in_maps(b, vp, capacity=capacity, **search, **descriptor)
            want = host_recognize(L, b, vp, capacity, search, **descriptor)
            assert same_candidates(got, want), (search, descriptor, capacity, got, want)
            assert len(got) <= capacity and summary.viewpoints == MAPPED
            assert summary.described == (MAPPED if capacity == 0 else 0)  # described once per setting, then kept
            mask = descriptor.get("type_mask", 3)
            assert list(summary.map_points) == [b.map(k).size if (mask >> k) & 1 else 0 for k in range(3)]
            assert list(summary.query_points) == [b.keypoints(k, which=2).size if (mask >> k) & 1 else 0 for k in range(3)]
    # the winner under the defaults
    found, _ = L.recognize_place_in_maps(b, vp, capacity=3)
    print("candidates:", [c[:4] for c in found])
    viewpoint, distance, shift, yaw, guess = found[0]
    off = float(np.linalg.norm(vp[viewpoint] - vp[QUERY]))
    sectors_off = min((shift - 15) % 60, (15 - shift) % 60)
    print("winner: viewpoint", viewpoint, "distance", distance, "shift", shift, "-", off, "m and", sectors_off, "sectors off; guess against the true pose", pose_diff(true, guess))
    assert off <= 1.0 and sectors_off <= 1
    T = np.eye(4)
    T[:2, :2] = [[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]]
    T[:3, 3] = vp[viewpoint]
    assert np.array_equal(guess, T)  # Translation(viewpoint) * Rz(yaw)
    # the call did not move the pose
    before = b.world_transform().copy()
    L.recognize_place_in_maps(b, vp)
    assert np.array_equal(b.world_transform(), before)
    end_b = go_on(L, b, guess)
    control = session_b(L, prefix, MapsOnDevice=on_device)
    end_control = go_on(L, control, true)
    wrong = session_b(L, prefix, MapsOnDevice=on_device)
    end_wrong = go_on(L, wrong, guess @ Rz(np.pi))
    mapping = P[QUERY + AFTER] @ Rz(np.pi / 2)
    d_m, d_rad = pose_diff(end_control, end_b)
    print("after +%d: recognised against control %.4f m %.5f rad (bound %.4f m %.5f rad); control against the mapping trajectory %s; recognised %s; "
          "started half a turn off against control %s" % (AFTER, d_m, d_rad, BOUND_M, BOUND_RAD, pose_diff(mapping, end_control), pose_diff(mapping, end_b),
                                                          pose_diff(end_control, end_wrong)))
    assert d_m <= BOUND_M and d_rad <= BOUND_RAD
    assert pose_diff(end_control, end_wrong)[1] > 3.0  # a yaw that is ignored cannot pass
    # refusals: after SetWorldTransformFromGuess the raw keypoints are gone; bad arguments; empty maps
    fresh = session_b(L, prefix, MapsOnDevice=on_device)
    fresh.set_world_transform_from_guess(true)
    with pytest.raises(L.LsaError) as e:
        L.recognize_place_in_maps(fresh, vp)
    assert e.value.code == L.E_STATE and "no frame has been added" in str(e.value)
    for bad in (dict(rings=0), dict(exclusion_radius=float("nan")), dict(capacity=-1), dict(max_distance=1.0, near_xyz=(0.0, float("inf"), 0.0))):
        with pytest.raises(L.LsaError) as e:
            L.recognize_place_in_maps(b, vp, **bad)
        assert e.value.code == L.E_ARG, bad
    broken = vp.copy()
    broken[3, 0] = np.nan
    for v in (broken, vp[:0]):
        with pytest.raises(L.LsaError) as e:
            L.recognize_place_in_maps(b, v)
        assert e.value.code == L.E_ARG
    empty = L.Slam(0, EgoMotion=3, MapUpdate=0, MapsOnDevice=on_device)
    pts, stamp = L.synth_frame(MODEL, 1001, QUERY)
    empty.add_frame(pts, stamp, 0)
    with pytest.raises(L.LsaError) as e:
        L.recognize_place_in_maps(empty, vp)
    assert e.value.code == L.E_STATE and "empty" in str(e.value)
    with pytest.raises(L.LsaError) as e:
        L.recognize_place_in_maps(L.Slam(0), vp)  # no frame at all
    assert e.value.code == L.E_STATE
    # without viewpoints: the positions of the trajectory, here the session's own two logged poses
    own, summary = L.recognize_place_in_maps(b, capacity=2, exclusion_radius=0.0)
    assert summary.viewpoints == b.trajectory()[0].shape[0] and len(own) == min(2, summary.viewpoints)
    for s in (b, control, wrong, fresh, empty):
        s.close()


def test_the_example_matches_the_python_front_end(tmp_path, L, mapped):
    """examples/slam_relocalization.cpp through the C++ mirror gives what the same calls give through the Python front end"""
    exe = build_example(tmp_path, "slam_relocalization")
    r = subprocess.run([exe, str(tmp_path / "m_"), str(MODEL), str(MAPPED), str(QUERY), str(AFTER)], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    extra = {}
    for words in (line.split()[1:] for line in lines if line.startswith("#")):
        extra.setdefault(words[0], []).append([float(v) for v in words[1:]])
    rows = np.array([[float(v) for v in line.split()] for line in lines if not line.startswith("#")])
    prefix, P = mapped
    vp = P[:, :3, 3].copy()
    b = session_b(L, prefix)
    found, summary = L.recognize_place_in_maps(b, vp, capacity=3)
    assert extra["described"] == [[summary.viewpoints, summary.described]] and len(extra["candidate"]) == len(found) >= 1
    for (viewpoint, distance, shift, yaw, _), printed in zip(found, extra["candidate"]):
        assert printed[0] == viewpoint and printed[2] == shift and printed[3] == yaw  # %.17g gives the double back
        assert np.float32(printed[1]) == distance                                   # %.9g the float
    assert np.allclose(extra["guess"][0], found[0][4][:3, 3], atol=1e-11, rtol=0) and np.allclose(extra["mapped"][0], vp[QUERY], atol=1e-11, rtol=0)
    b.set_world_transform_from_guess(found[0][4])
    assert rows.shape == (AFTER, 4)
    for i, f in enumerate(range(QUERY + 1, QUERY + 1 + AFTER)):
        pts, stamp = L.synth_frame(MODEL, 1001, f)
        b.add_frame(turned(pts), stamp, 1 + i)
        assert rows[i, 0] == f and np.allclose(rows[i, 1:4], b.world_transform()[:3, 3], atol=1e-9, rtol=0)
    b.close()


# ---- the frame path does not notice ------------------------------------------------------------------------------------------------
def snapshot(L, s):
    P, t, cov = s.trajectory()
    return (s.world_transform().tobytes(), s.covariance().tobytes(), [s.map(k).tobytes() for k in (L.EDGE, L.PLANE)],
            [s.target_submap(k).tobytes() for k in (L.EDGE, L.PLANE)], P.tobytes(), t.tobytes(), cov.tobytes(), s.logged_frames(),
            s.get_param("NbrFrameProcessed"))


@pytest.mark.parametrize("on_device", [1, 0])
def test_the_frame_path_does_not_notice_a_recognition(L, on_device):
    frames = [L.synth_frame(MODEL, 1000, f) for f in range(12)]

    def run(recognize):
        s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, MapsOnDevice=on_device)
        shots = []
        for f, (pts, stamp) in enumerate(frames):
            s.add_frame(pts, stamp, f)
            if f in (6, 9):
                # (both runs read the same state through the same getters the same number of times: the recognitions and
                #  the refused calls are the only difference between them)
                before = snapshot(L, s)
                if recognize:
                    found, summary = L.recognize_place_in_maps(s, capacity=3, exclusion_radius=0.4)
                    assert len(found) >= 1 and summary.described == f + 1
                    assert L.recognize_place_in_maps(s, capacity=3, exclusion_radius=0.4)[1].described == 0
                    L.recognize_place_in_maps(s, rings=32, sectors=120, type_mask=7)
                    with pytest.raises(L.LsaError):
                        L.recognize_place_in_maps(s, rings=33)
                    with pytest.raises(L.LsaError):
                        L.recognize_place_in_maps(s, np.array([[np.nan, 0.0, 0.0]]))
                assert snapshot(L, s) == before
            if f >= 7:
                shots.append(snapshot(L, s))
        assert s.get_param("DeviceSolveFallbacks") == 0
        s.close()
        return shots

    assert run(True) == run(False)
