"""DenseMapHost.carve, the definition of the dense map's free-space carving (lidarslam_amd/_dense_map.py): the walk, the
counting, the filtered exports, prune and reproject.  Numpy alone: no GPU, no native library.  Cases: tests/dense_carve_cases.py."""
import numpy as np
import pytest

import dense_carve_cases as K
import dense_map_cases as M
from lidarslam_amd._dense_map import DenseMapHost, dense_index_keys, dense_voxel_keys


def state(h, min_frames=1, ratio=-1.0):
    pts, vox = h.get(min_frames, ratio)
    return pts.tobytes(), vox.tobytes(), h.sources(min_frames, ratio).tobytes(), h.misses(min_frames, ratio).tobytes()


def end_points(name):
    """(i0, i1) of the ray by the definition's own first five statements, or None"""
    o, p, kw = K.RAY_CASES[name]
    o, p = np.asarray(o, np.float32).astype(np.float64), np.asarray(p, np.float32).astype(np.float64)
    d = p - o
    length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    t = min(length - kw.get("margin_leaves", 2.0) * K.LEAF, kw.get("max_range", 30.0))
    if not (np.isfinite(o).all() and np.isfinite(p).all() and t > 0):
        return None
    e = o + d * (t / length)
    i0, i1 = np.floor(o / K.LEAF), np.floor(e / K.LEAF)
    if not all(-(1 << 20) <= v < (1 << 20) for v in list(i0) + list(i1)):
        return None
    return tuple(int(v) for v in i0), tuple(int(v) for v in i1)


# ---- the walk -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.RAY_CASES))
def test_the_walk_ends_in_the_end_voxel_is_connected_and_has_the_announced_length(name):
    visited, ends = K.walk(name), end_points(name)
    assert (visited is None) == (ends is None) == (name in K.NO_RAY)
    if visited is None:
        return
    i0, i1 = ends
    assert visited[0] == i0 and visited[-1] == i1
    assert len(visited) == 1 + sum(abs(a - b) for a, b in zip(i0, i1))
    for a, b in zip(visited, visited[1:]):
        assert sorted(abs(x - y) for x, y in zip(a, b)) == [0, 0, 1]  # 6-connected
    # every visited voxel's centre within 0.7 leaves (Chebyshev) of the segment
    o = np.asarray(K.RAY_CASES[name][0], np.float32).astype(np.float64)
    p = np.asarray(K.RAY_CASES[name][1], np.float32).astype(np.float64)
    s = np.linspace(0.0, 1.0, 4001)[:, None]
    seg = o + (p - o) * s
    for v in visited[:: max(1, len(visited) // 40)]:
        c = (np.asarray(v) + 0.5) * K.LEAF
        assert np.abs(seg - c).max(axis=1).min() <= 0.7 * K.LEAF + 1e-9, v


def test_named_walks():
    assert K.walk("axis+x") == [(i, 0, 0) for i in range(5)]  # 3.0 long less the margin of 1.0: ends at 2.125
    assert K.walk("axis-z") == [(0, 0, -i) for i in range(5)]  # ends at -1.875: voxel -4
    assert K.walk("one_voxel") == [(0, 0, 0)] == K.walk("over_margin")
    assert len(K.walk("long")) > 60 and len(K.walk("short_range")) < 12
    assert K.walk("stays_inside")[-1] == ((1 << 20) - 1, 0, 0) and K.walk("low_edge")[-1] == (-(1 << 20), 0, 0)


@pytest.mark.parametrize("name", sorted(K.TIES))
def test_ties_go_to_x_before_y_before_z(name):
    assert K.walk(name) == K.TIES[name]


def test_random_rays_end_where_they_should():
    """lattice-aligned and random rays: the walk of all rays at once is the walk of each alone, and ends in i1"""
    rng = np.random.default_rng(1)
    p = np.concatenate([rng.uniform(-9, 9, (300, 3)), rng.integers(-40, 40, (300, 3)) * M.STEP])
    o = np.concatenate([rng.uniform(-2, 2, (300, 3)), rng.integers(-8, 8, (300, 3)) * M.STEP]).astype(np.float32)
    pts = M.cloud(p)
    together = K.walks(pts, o, margin_leaves=0.0)
    for j in range(0, 600, 7):
        assert together[j] == K.walks(pts[j : j + 1], o[j : j + 1], margin_leaves=0.0)[0]
    keys, ok = dense_voxel_keys(pts, K.LEAF)
    for j, w in enumerate(together):
        if w is not None:  # margin 0: the ray ends in the point's own voxel
            assert ok[j] and int(dense_index_keys([w[-1]])[0]) == int(keys[j])
            assert all(sorted(abs(x - y) for x, y in zip(a, b)) == [0, 0, 1] for a, b in zip(w, w[1:]))


# ---- counting -----------------------------------------------------------------------------------------------------------------
def line_map():
    """voxels (0..7, 0, 0) and (0..7, 1, 0), made in ordinal 0"""
    h = DenseMapHost(K.LEAF)
    h.insert(K.voxel_points([(i, j, 0) for j in range(2) for i in range(8)]), 0)
    return h


def along_x(n, y=0.125):
    """n rays from (0.125, y, 0.125) to x = 3.9, margin 0: voxels 0..7 of row 0"""
    pts = M.cloud([[3.9, y, 0.125]] * n)
    return pts, np.array([[0.125, y, 0.125]], np.float32)


def test_many_rays_count_once_and_again_in_the_next_ordinal():
    h = line_map()
    before = h.get()
    pts, org = along_x(50)
    h.carve(pts, org, 1, margin_leaves=0.0)
    assert h.rays == 50 and h.misses().tolist() == [1] * 8 + [0] * 8
    h.carve(pts, org, 1, margin_leaves=0.0)  # two calls under one ordinal
    assert h.rays == 100 and h.misses().tolist() == [1] * 8 + [0] * 8
    h.carve(pts[:1], org, 2, margin_leaves=0.0)
    assert h.misses().tolist() == [2] * 8 + [0] * 8
    after = h.get()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()  # get() of today, to the byte
    assert h.size() == 16 and h.skipped == 0
    with pytest.raises(ValueError):
        h.carve(pts, org, 1)  # ordinals must not decrease
    with pytest.raises(ValueError):
        h.carve(pts, org, -(1 << 31))


def test_a_voxel_hit_in_the_same_ordinal_is_not_counted():
    h = line_map()
    h.insert(K.voxel_points([(3, 0, 0), (20, 0, 0)]), 1)
    pts, org = along_x(3)
    h.carve(pts, org, 1, margin_leaves=0.0)
    assert h.misses().tolist()[:16] == [1, 1, 1, 0, 1, 1, 1, 1] + [0] * 8
    h.carve(pts, org, 2, margin_leaves=0.0)
    assert h.misses().tolist()[:16] == [2, 2, 2, 1, 2, 2, 2, 2] + [0] * 8


def test_the_order_of_the_rays_does_not_matter_and_stride_takes_every_kth():
    base = DenseMapHost(K.LEAF)
    pts = K.ray_cloud(500, seed=2)
    base.insert(pts, 0)
    org = (np.random.default_rng(3).uniform(-1, 1, (500, 3))).astype(np.float32)
    perm = np.random.default_rng(4).permutation(500)
    a, b = DenseMapHost(K.LEAF), DenseMapHost(K.LEAF)
    for h in (a, b):
        h.insert(pts, 0)
    a.carve(pts, org, 1)
    b.carve(pts[perm], org[perm], 1)
    assert state(a) == state(b) and a.rays == b.rays and a.misses().sum() > 100
    for stride in (2, 7, 501):
        c, d = DenseMapHost(K.LEAF), DenseMapHost(K.LEAF)
        c.insert(pts, 0), d.insert(pts, 0)
        c.carve(pts, org, 1, stride=stride)
        d.carve(pts[::stride], org[::stride], 1)
        assert state(c) == state(d) and 0 < c.rays == d.rays <= len(pts[::stride])  # (a point nearer than the margin casts none)
    one = DenseMapHost(K.LEAF)
    one.insert(pts, 0)
    one.carve(pts, org[:1], 1)
    rep = DenseMapHost(K.LEAF)
    rep.insert(pts, 0)
    rep.carve(pts, np.repeat(org[:1], 500, axis=0), 1)
    assert state(one) == state(rep)  # (1, 3) origins are (n, 3) of the same row


# ---- the scene ----------------------------------------------------------------------------------------------------------------
def test_the_scene_keeps_the_wall_and_loses_the_object():
    h, wall, obj = K.host_scene()
    wall_keys, obj_keys = set(dense_index_keys(wall).tolist()), set(dense_index_keys(obj).tolist())
    assert len(wall_keys) == 169 and len(obj_keys) == 8 * 4 - 4 * 3 and h.size() == len(wall_keys) + len(obj_keys)
    pts, vox = h.get(1, 1.0)
    assert set(vox["key"].tolist()) == wall_keys  # every wall voxel and no object voxel
    assert h.misses(1, 1.0).tolist() == [0] * len(wall_keys)
    vox = h.get()[1]
    every = dict(zip(vox["key"].tolist(), zip(h.misses().tolist(), vox["frames"].tolist(), vox["first_frame"].tolist())))
    assert all(every[k][0] > every[k][1] for k in obj_keys), "the wall's rays do not cover the object"
    # seen through in every frame since it was made that did not hit it
    assert all(every[k][0] == K.SCENE_FRAMES - every[k][2] - every[k][1] for k in obj_keys)
    kept = state(h, 1, 1.0)
    assert h.prune(1, 1.0) == len(obj_keys) == h.pruned
    assert state(h) == kept and h.size() == len(wall_keys) and h.skipped == 0 and h.dropped == 0
    assert h.prune(1, 1.0) == 0


def test_the_filter_at_four_ratios():
    h, wall, obj = K.host_scene()
    pts, vox = h.get()
    misses, frames = h.misses().astype(np.float64), vox["frames"].astype(np.float64)
    assert state(h, 1, -1.0) == state(h) and h.get(1, -1.0)[1].tobytes() == vox.tobytes()
    sizes = []
    for ratio in K.RATIOS:
        keep = np.ones(len(vox), bool) if ratio < 0 else misses <= ratio * frames
        got = h.get(1, ratio)
        assert got[1].tobytes() == vox[keep].tobytes() and got[0].tobytes() == pts[keep].tobytes()
        assert h.misses(1, ratio).tobytes() == h.misses()[keep].tobytes() and h.sources(1, ratio).tobytes() == h.sources()[keep].tobytes()
        sizes.append(int(keep.sum()))
    assert sizes == [169, 169, 169, h.size()]
    # a voxel with as many misses as frames stays at ratio 1 and goes at 0.5; min_frames still applies
    g = line_map()
    p, o = along_x(1)
    g.carve(p, o, 1, margin_leaves=0.0)
    assert len(g.get(1, 1.0)[1]) == 16 and len(g.get(1, 0.5)[1]) == 8 and len(g.get(2, 1.0)[1]) == 0


# ---- reproject ----------------------------------------------------------------------------------------------------------------
def test_reproject_carries_the_misses_and_leaves_a_map_never_carved_as_before():
    calls = M.wall_and_mover()[0]
    a, b = M.host_map(DenseMapHost, calls), M.host_map(DenseMapHost, calls)
    shift = np.eye(4)
    shift[0, 3] = 0.25
    D = np.stack([np.eye(4).ravel()] * 4 + [shift.ravel()] * 4)
    b.carve(M.cloud([[50.0, 50.0, 50.0]]), [[49.0, 49.0, 49.0]], 7)  # a ray that meets nothing
    assert a.reproject(D) == b.reproject(D) == 0
    assert state(a)[:3] == state(b)[:3] and not a.misses().any() and not b.misses().any()
    # two voxels brought into one key: misses add up, the later miss ordinal stays
    h = DenseMapHost(K.LEAF)
    h.insert(K.voxel_points([(0, 0, 0), (5, 0, 0)]), 0)
    h.insert(K.voxel_points([(1, 0, 0)]), 1)
    p, o = along_x(1)
    h.carve(p, o, 2, margin_leaves=0.0)
    h.carve(M.cloud([[0.9, 0.125, 0.125]]), o, 3, margin_leaves=0.0)  # voxels 0 and 1 again
    assert h.misses().tolist() == [2, 2, 1]
    move = np.eye(4)
    move[0, 3] = -0.5
    assert h.reproject(np.stack([np.eye(4).ravel(), move.ravel()])) == 0  # the voxel of ordinal 1 moves onto voxel 0
    assert h.size() == 2 and h.misses().tolist() == [4, 1] and h.get()[1]["count"].tolist() == [2, 1]
    h.carve(M.cloud([[0.4, 0.125, 0.125]]), o, 3, margin_leaves=0.0)  # counted in ordinal 3 already
    assert h.misses().tolist() == [4, 1]
    h.carve(M.cloud([[0.4, 0.125, 0.125]]), o, 4, margin_leaves=0.0)
    assert h.misses().tolist() == [5, 1]


def test_clear_forgets_everything():
    h, _, _ = K.host_scene()
    h.prune(1, 1.0)
    assert h.rays > 0 and h.pruned > 0
    h.clear()
    assert h.size() == 0 and h.rays == 0 and h.pruned == 0 and len(h.misses()) == 0
