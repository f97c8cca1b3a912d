"""The dense map's floor plan on the device (lidarslam_amd/csrc/lsa_dense_grid.hip: k_dense_grid_*) against the host statement
(DenseMapHost.grid), on the bytes of the info, of all 20 of every record with its NaNs and of every state: the cases and
queries of tests/dense_grid_cases.py, long probe sequences and the smallest table, the map after growth, re-projection,
carving, pruning and a clear, repeated calls, the capacity rule, the cell cap, the pipeline, the files."""
import os

import numpy as np
import pytest

import dense_carve_cases as K
import dense_grid_cases as G
import dense_map_cases as M

pytestmark = pytest.mark.gpu

PIPE_LEAF = 0.2


def same(d, h, **q):
    """the device's grid of query q is the host's, byte for byte; returns it"""
    got = d.grid(**q)
    G.same_grid(got, h.grid(**q))
    return got


def pair(L, ctx, leaf, steps, **params):
    return G.play(L.DenseMap(ctx, leaf, **params), steps), G.play(L.DenseMapHost(leaf), steps)


# ---- the cases of the definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.CASES))
def test_every_case_and_query(L, gpu_ctx, name):
    leaf, steps, queries, params = G.CASES[name]()
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    assert K.same_state(d, h) == h.size() > 0
    cells = sum(same(d, h, **q)[2].size for q in queries)
    assert cells > 0
    assert K.same_state(d, h) == h.size()  # read-only
    d.close()


def test_probe_stress_and_the_smallest_table(L, gpu_ctx):
    leaf, pts = G.scattered(seed=4, n=400)
    for stress in (0, 1):
        d, h = pair(L, gpu_ctx, leaf, [("insert", pts[:250], 0), ("insert", pts[150:], 1)], InitialCapacity=64, ProbeStress=stress)
        assert d.get_param("Rehashes") >= 1
        for q in G.SCATTERED_QUERIES + [dict(min_frames=2), dict(window=G.WINDOWS["inside"], cell_leaves=1)]:
            assert same(d, h, **q)[2].size > 0
        d.close()
    d, h = pair(L, gpu_ctx, G.LEAF, G.pole()[1], InitialCapacity=64, ProbeStress=1)
    assert d.get_param("Capacity") == 64
    same(d, h, cell_leaves=1), same(d, h, cell_leaves=3, ground_radius=16)
    d.close()


# ---- the table after what changes it ------------------------------------------------------------------------------------------
def test_after_growth_reprojection_carving_pruning_and_a_clear(L, gpu_ctx):
    calls = M.growth_calls()
    d, h = pair(L, gpu_ctx, M.LEAF, [("insert", pts, f) for pts, f in calls[:4]], InitialCapacity=64, **G.CARVE_PARAMS)
    assert d.get_param("Rehashes") >= 3
    queries = [dict(), dict(cell_leaves=1, ground_radius=1, min_height=0.5, max_height=4.0), dict(cell_leaves=3, min_frames=2), dict(window=(-3.0, -2.0, 4.4, 1.9), max_height=5.0)]
    before = [same(d, h, **q) for q in queries]
    D = np.stack([np.eye(4)] * 4)
    D[1, 0, 3], D[2, 1, 3], D[3, 2, 3] = 0.5, -0.5, 1.0
    assert d.reproject(D) == h.reproject(D.reshape(-1, 16))
    moved = [same(d, h, **q) for q in queries]
    assert moved[0][1].tobytes() != before[0][1].tobytes()
    rays = K.ray_cloud(400, seed=3, reach=5.0)
    for m in (d, h):
        G.play(m, [("carve", rays, K.SENSOR, 7), ("carve", rays[::-1], K.SENSOR, 8)])
    assert h.misses().sum() > 50
    for q in queries:
        same(d, h, **dict(q, max_miss_ratio=0.5))
    assert d.prune(1, 0.5) == h.prune(1, 0.5) > 0
    for q in queries:
        same(d, h, **q)
    d.clear(), h.clear()
    assert d.grid()[1].shape == h.grid()[1].shape == (0, 0)
    assert same(d, h, window=(0.0, 0.0, 2.0, 1.0))[2].tolist() == [[-1] * 3] * 2  # a window is answered whatever the map holds
    for m in (d, h):
        G.play(m, [("insert", calls[4][0], 0)])
    for q in queries:
        same(d, h, **q)
    d.close()


def test_repeated_calls_and_the_capacity_rule(L, gpu_ctx):
    leaf, steps, _, params = G.CASES["wide65"]()
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    q = dict(ground_radius=1)
    first = same(d, h, **q)
    again = d.grid(**q)
    assert G.same_grid(again, first) == 195 and G.same_grid(d.grid(**q), first) and d.get_param("GridSeconds") > 0
    assert K.same_state(d, h) == h.size()  # read-only
    # as the other exports: the count whatever the capacity, nothing written past it, the info either way
    p = L.DenseGridParams(min_height=0.2, max_height=2.0, max_miss_ratio=-1.0, cell_leaves=2, ground_radius=1, min_obstacle_voxels=1, min_frames=1)
    import ctypes as C

    def call(cells, state, cap):
        info = L.DenseGridInfo()
        n = d.L.lsa_dense_map_get_grid(d.h, C.byref(p), C.byref(info), L.ptr(cells) if cells is not None else None, L.ptr(state) if state is not None else None, cap)
        return n, (info.cx0, info.cy0, info.width, info.height, info.resolution, info.origin_x, info.origin_y)

    want = tuple(first[0].tolist())
    cells, state = np.zeros(9, L.dense_cell_dtype), np.full(9, 77, np.int8)
    cells["floor_voxels"][7:] = 0xABCDEF
    assert call(cells, state, 7) == (195, want)
    assert cells[:7].tobytes() == first[1].reshape(-1)[:7].tobytes() and (cells["floor_voxels"][7:] == 0xABCDEF).all()
    assert state[:7].tobytes() == first[2].reshape(-1)[:7].tobytes() and (state[7:] == 77).all()
    assert call(None, None, 0) == (195, want) and call(None, state, 9)[0] == 195 and state.tobytes() == first[2].reshape(-1)[:9].tobytes()
    assert call(cells, None, 9)[0] == 195 and cells.tobytes() == first[1].reshape(-1)[:9].tobytes()
    assert call(cells, state, -1)[0] == L.E_ARG
    info = L.DenseGridInfo()
    assert d.L.lsa_dense_map_get_grid(d.h, None, C.byref(info), None, None, 0) == L.E_ARG and d.L.lsa_dense_map_get_grid(d.h, C.byref(p), None, None, None, 0) == L.E_ARG
    d.close()


def test_refusals_leave_the_state(L, gpu_ctx):
    leaf, steps, _, params = G.CASES["car"]()
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    bad = [dict(cell_leaves=0), dict(cell_leaves=65), dict(ground_radius=-1), dict(ground_radius=17), dict(min_height=-0.1), dict(min_height=2.0), dict(min_height=3.0),
           dict(max_height=np.inf), dict(min_height=np.nan), dict(min_obstacle_voxels=0), dict(window=(1.0, 0.0, 0.5, 1.0)), dict(window=(0.0, 1.0, 1.0, 0.5)),
           dict(window=(0.0, 0.0, np.inf, 1.0)), dict(window=(np.nan, 0.0, 1.0, 1.0))]
    for q in bad:
        with pytest.raises(L.LsaError) as e:
            d.grid(**q)
        assert e.value.code == L.E_ARG, q
        with pytest.raises(ValueError):
            h.grid(**q)
    with pytest.raises(L.LsaError) as e:
        d.save_grid("no", cell_leaves=0)
    assert e.value.code == L.E_ARG and not os.path.exists("no.pgm")
    for name, value in (("GridMaxCells", 0), ("GridMaxCells", 2.0**28 + 1), ("GridMaxCells", 2.5)):
        with pytest.raises(L.LsaError):
            d.set(name, value)
    assert K.same_state(d, h) == h.size() and K.same_state(d, h, 1, 1.0) < h.size()
    same(d, h, cell_leaves=1, max_miss_ratio=1.0)
    d.close()


def test_the_cell_cap_refuses_before_anything_is_allocated(L, gpu_ctx):
    d, h = pair(L, gpu_ctx, G.LEAF, [("insert", G.far_apart(), 0)])
    assert d.get_param("GridMaxCells") == 2.0**24
    for q in (dict(), dict(cell_leaves=1), dict(cell_leaves=64, ground_radius=16)):
        with pytest.raises(L.LsaError) as e:
            d.grid(**q)
        assert e.value.code == L.E_CAPACITY and "GridMaxCells" in str(e.value), q
        with pytest.raises(OverflowError):
            h.grid(**q)
    with pytest.raises(L.LsaError) as e:
        d.save_grid("no")
    assert e.value.code == L.E_CAPACITY and not os.path.exists("no.pgm")
    assert K.same_state(d, h) == 2
    # the next call still works: a window, and the whole under a cap it fits
    same(d, h, window=(-1.0, -1.0, 1.0, 1.0))
    near = -(L.DENSE_INDEX_RANGE // 2) * G.LEAF
    assert same(d, h, cell_leaves=1, window=(near - 1.0, near - 1.0, near + 1.0, near + 1.0))[2].tolist().count([-1] * 4 + [0] + [-1] * 4) == 1
    d.set("GridMaxCells", 8)
    with pytest.raises(L.LsaError) as e:
        d.grid(window=(0.0, 0.0, 1.0, 1.0))  # 3 x 3 cells
    assert e.value.code == L.E_CAPACITY
    with pytest.raises(OverflowError):
        h.grid(window=(0.0, 0.0, 1.0, 1.0), max_cells=8)
    d.set("GridMaxCells", 9)
    G.same_grid(d.grid(window=(0.0, 0.0, 1.0, 1.0)), h.grid(window=(0.0, 0.0, 1.0, 1.0), max_cells=9))
    d.close()


# ---- the pipeline --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driven(L):
    """a short VLP-16 drive with the dense map and carving on; the host statement fed the registered frames"""
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, DenseMapCarve=1, DenseMapCarveRange=12.0, DenseMapCarveStride=3)
    h = L.DenseMapHost(PIPE_LEAF)
    for f in range(6):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
        h.insert(s.registered_frame().copy(), f)
    yield s, h
    s.close()


def test_the_pipelines_grid_is_the_host_statement_of_its_registered_frames(L, driven):
    s, h = driven
    assert h.skipped == 0 and L.dense_map_size(s) == h.size() > 5000
    whole = L.dense_map_grid(s)
    G.same_grid(whole, h.grid())
    G.same_grid(L.dense_map_grid(s, cell_leaves=1, ground_radius=4, min_frames=2), h.grid(cell_leaves=1, ground_radius=4, min_frames=2))
    x, y = s.world_transform()[:2, 3]
    local = L.dense_map_grid(s, half_extent=10.0)
    G.same_grid(local, h.grid(window=(x - 10.0, y - 10.0, x + 10.0, y + 10.0)))
    assert local[1].shape in ((50, 50), (51, 51), (50, 51), (51, 50))
    # the street canyon of the synthetic drive: the road at z = -1.8 ahead of the vehicle, facades at y = +-8
    info, cells, state = whole
    res, ox, oy = float(info["resolution"]), float(info["origin_x"]), float(info["origin_y"])
    cx = ox + res * (np.arange(int(info["width"])) + 0.5)
    cy = oy + res * (np.arange(int(info["height"])) + 0.5)
    road = state[np.ix_(np.abs(cy - y) < 1.0, (cx > x + 6.5) & (cx < x + 9.5))]
    facade = state[np.ix_((cy > 8.0) & (cy < 8.4), np.abs(cx - x) < 5.0)]
    print("road", np.unique(road, return_counts=True), "facade", np.unique(facade, return_counts=True))
    assert (road == 0).sum() > 0 and (road == 100).sum() == 0  # seen floor is free, nothing stands on the road
    assert facade.size > 0 and (facade == 100).mean() > 0.5
    seen = cells["elevation"][~G.absent(cells, "elevation")]
    assert abs(float(np.median(cells["ground"][state == 0])) + 1.8) < 0.1 and seen.size > 1000
    # the filters of the export: what was seen through is left out here as there
    filtered = L.dense_map_grid(s, max_miss_ratio=1.0)
    kept_pts, kept = L.dense_map_filtered(s, 1, 1.0)
    assert 0 < len(kept) < h.size()
    G.same_grid(filtered, L.dense_grid(kept_pts, kept["key"], PIPE_LEAF))
    with pytest.raises(L.LsaError) as e:
        L.dense_map_grid(s, cell_leaves=0)
    assert e.value.code == L.E_ARG
    s.set_param("DenseMapGridMaxCells", 16)
    with pytest.raises(L.LsaError) as e:
        L.dense_map_grid(s)
    assert e.value.code == L.E_CAPACITY and s.get_param("DenseMapGridMaxCells") == 16
    s.set_param("DenseMapGridMaxCells", 2**24)
    G.same_grid(L.dense_map_grid(s), whole)


def test_off_the_calls_refuse_and_before_the_first_frame_the_map_is_empty(L):
    s = L.Slam(0, EgoMotion=3)
    for call in (lambda: L.dense_map_grid(s), lambda: L.save_dense_map_grid(s, "no")):
        with pytest.raises(L.LsaError) as e:
            call()
        assert e.value.code == L.E_STATE
    assert not os.path.exists("no.pgm")
    s.close()
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF)
    info, cells, state = L.dense_map_grid(s)
    assert cells.shape == (0, 0) and float(info["resolution"]) == 2 * PIPE_LEAF
    G.same_grid(L.dense_map_grid(s, window=(0.0, 0.0, 1.0, 1.0)), L.DenseMapHost(PIPE_LEAF).grid(window=(0.0, 0.0, 1.0, 1.0)))
    pts, stamp = L.synth_frame(16, 1000, 0)
    s.add_frame(pts, stamp, 0)
    assert L.dense_map_grid(s)[2].size > 1000
    s.close()


# ---- files -----------------------------------------------------------------------------------------------------------------------
def test_saved_files_are_the_returned_arrays(L, gpu_ctx, driven, tmp_path):
    leaf, steps, queries, params = G.CASES["car"]()
    d, h = pair(L, gpu_ctx, leaf, steps, **params)
    G.play(d, [("insert", G.at([[1, 1, 3]]), 6)]), G.play(h, [("insert", G.at([[1, 1, 3]]), 6)])  # the rows differ
    info, cells, state = same(d, h, **queries[0])
    prefix = str(tmp_path / "plan")
    assert d.save_grid(prefix, **queries[0]) == 27
    back, resolution, origin = L.read_occupancy_pgm(prefix)
    assert back.tobytes() == state.tobytes() and (resolution, origin) == (float(info["resolution"]), (float(info["origin_x"]), float(info["origin_y"])))
    theirs = str(tmp_path / "host")
    assert L.write_occupancy_pgm(theirs, info, state) == 27
    assert open(prefix + ".pgm", "rb").read() == open(theirs + ".pgm", "rb").read()
    assert open(prefix + ".yaml").read() == open(theirs + ".yaml").read().replace("host.pgm", "plan.pgm")
    assert d.save_grid(str(tmp_path / "none"), min_frames=9) == 0 and not os.path.exists(str(tmp_path / "none.pgm"))
    with pytest.raises(L.LsaError) as e:
        d.save_grid(str(tmp_path / "missing" / "plan"))
    assert e.value.code == L.E_ARG and "missing" in str(e.value)
    d.close()
    # the pipeline's: unknown cells among them, an origin that is no round number
    s, h = driven
    prefix = str(tmp_path / "street")
    info, _, state = L.dense_map_grid(s, max_miss_ratio=1.0)
    assert L.save_dense_map_grid(s, prefix, max_miss_ratio=1.0) == state.size
    back, resolution, origin = L.read_occupancy_pgm(prefix)
    assert back.tobytes() == state.tobytes() and set(np.unique(back).tolist()) == {-1, 0, 100}
    assert (resolution, origin) == (float(info["resolution"]), (float(info["origin_x"]), float(info["origin_y"])))
    # the host-only writer of the C ABI gives the same files
    again = str(tmp_path / "again")
    cinfo = L.DenseGridInfo(*[info[n].item() for n in L.dense_grid_info_dtype.names])
    import ctypes as C

    assert L.lib().lsa_occupancy_write(os.fsencode(again), C.byref(cinfo), L.ptr(np.ascontiguousarray(state))) == 0
    assert open(again + ".pgm", "rb").read() == open(prefix + ".pgm", "rb").read()
