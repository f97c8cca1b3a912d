"""DenseMapHost.reproject and DenseMapHost.sources (lidarslam_amd/_dense_map.py), the statement the device's re-projection is
held to: the source per voxel, the move, the new keys, the merge rule, the clamp, the drops, and where it agrees exactly with a
rebuild from the moved frames.  Cases: tests/dense_reproject_cases.py.  No GPU, no native library."""
import numpy as np
import pytest

import dense_map_cases as K
import dense_reproject_cases as R


@pytest.fixture(scope="module")
def H(L):
    return L.DenseMapHost


def voxel(h, index):
    """(point, record, source) of the voxel at `index`"""
    pts, vox = h.get()
    j = int(np.flatnonzero(vox["key"] == K.key_of(index))[0])
    return pts[j], vox[j], int(h.sources()[j])


def other_bytes(pts):
    """the 20 bytes of every point that a re-projection keeps"""
    return [pts[n].tobytes() for n in pts.dtype.names if n not in ("x", "y", "z")]


# ---- the source ------------------------------------------------------------------------------------------------------------------
def test_sources_after_inserts(H):
    h = K.host_map(H, K.ties())
    assert h.sources().tolist() == [0, 1] and h.sources().dtype == np.int32  # nine against nine stays with frame 0; five replaces four
    h = K.host_map(H, K.nan_intensity())
    assert h.sources().tolist() == [0, 3, 0]  # a later NaN replaces nothing, any number replaces a NaN
    h = K.host_map(H, K.signed_zero())
    assert h.sources().tolist() == [0, 1, 0]  # only +0.0 against -0.0 is strictly greater
    h = K.host_map(H, K.same_ordinal_twice())
    assert h.sources().tolist() == [4, 4, 4] and h.sources(2).tolist() == [4]  # aligned with get(min_frames)
    assert len(h.get(2)[1]) == 1 and H(K.LEAF).sources().size == 0


# ---- the move and the keys -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.IDENTITY_KEEPS)
def test_the_identity_keeps_points_records_and_sources(H, name):
    calls, D, first = R.CASES[name]()
    h = K.host_map(H, calls)
    before = R.state(h), R.state(h, 2)
    assert h.reproject(D, first) == 0 and h.dropped == 0
    assert (R.state(h), R.state(h, 2)) == before


def test_a_minus_zero_comes_out_plus_zero_under_the_identity(H):
    calls, _ = K.negative_coordinates()
    h = K.host_map(H, calls)
    before_pts, before_vox = h.get()
    assert np.signbit(before_pts["z"]).any()  # voxel 0 holds the point with z = -0.0
    assert h.reproject(R.identity()) == 0
    pts, vox = h.get()
    assert vox.tobytes() == before_vox.tobytes()
    for a in ("x", "y", "z"):
        assert (pts[a] == before_pts[a]).all() and not np.signbit(pts[a][pts[a] == 0]).any()
    assert other_bytes(pts) == other_bytes(before_pts)


def test_a_translation_of_one_leaf_shifts_the_keys_only(H):
    for name in ("one_leaf_wall", "one_leaf_ties"):
        calls, D, first = R.CASES[name]()
        h = K.host_map(H, calls)
        bp, bv = h.get()
        bs = h.sources()
        assert h.reproject(D, first) == 0
        pts, vox = h.get()
        shift = (2 << 42) - (1 << 21) + 1  # one leaf up x, one down y, two up z
        assert (vox["key"].astype(np.int64) - bv["key"].astype(np.int64) == shift).all()  # the order is kept: one shift for all
        for f in ("count", "frames", "first_frame", "last_frame"):
            assert (vox[f] == bv[f]).all()
        assert (h.sources() == bs).all()
        assert (pts["x"] == bp["x"] + 0.5).all() and (pts["y"] == bp["y"] - 0.5).all() and (pts["z"] == bp["z"] + 1.0).all()
        assert other_bytes(pts) == other_bytes(bp)


# ---- the merge rule --------------------------------------------------------------------------------------------------------------
def test_merged_voxels_add_counts_and_span_the_frames(H):
    h, dropped = R.reprojected_host(H, R.merge_counts())
    assert dropped == 0 and h.size() == 1
    p, v, s = voxel(h, (0, 0, 0))
    assert (v["count"], v["frames"], v["first_frame"], v["last_frame"]) == (6, 3, 0, 5)  # 1 + 2 frames under a span of 6
    assert s == 0 and p["intensity"] == 9 and (p["x"], p["y"], p["z"]) == (0.125, 0.0, 0.0)


def test_the_frames_of_a_merged_voxel_never_exceed_its_span(H):
    h, _ = R.reprojected_host(H, R.merge_frames_cap_binds())
    assert h.size() == 1
    p, v, s = voxel(h, (0, 0, 0))
    assert (v["count"], v["frames"], v["first_frame"], v["last_frame"]) == (6, 3, 0, 2)  # 3 + 3 frames, capped at the span
    assert s == 0 and p["intensity"] == 9


def test_intensity_then_source_then_old_key_decide_the_point(H):
    calls, D, first = R.merge_intensity()
    h, _ = R.reprojected_host(H, (calls, D, first))
    p, v, s = voxel(h, (0, 0, 0))
    assert s == 1 and p["intensity"] == 6 and (p["x"], p["y"], p["z"]) == (0.125, 0.25, 0.375) and p["time"] == calls[1][0]["time"][0]
    assert (v["count"], v["frames"], v["first_frame"], v["last_frame"]) == (2, 2, 0, 1)

    h, _ = R.reprojected_host(H, R.merge_source_tie())
    p, v, s = voxel(h, (0, 0, 0))
    assert s == 1 and (p["x"], p["y"], p["z"]) == (0.125, 0.25, 0.375)  # six against six: ordinal 1 before ordinal 2
    assert (v["count"], v["frames"], v["first_frame"], v["last_frame"]) == (3, 3, 0, 2)

    h, _ = R.reprojected_host(H, R.merge_signed_source_tie())
    p, v, s = voxel(h, (0, 0, 0))
    assert s == -1 and p["y"] == 0.25 and (v["first_frame"], v["last_frame"], v["frames"]) == (-1, 1, 2)

    calls, D, first = R.merge_key_tie()
    h, _ = R.reprojected_host(H, (calls, D, first))
    assert h.size() == 3
    for index, xyz in (((1, 0, 0), (0.5, 0.125, 0.125)), ((8, 2, 0), (4.125, 1.0, 0.125)), ((-6, -6, 0), (-2.875, -2.875, 0.0))):
        p, v, s = voxel(h, index)
        assert (p["x"], p["y"], p["z"]) == xyz and v["count"] == 2 and v["frames"] == 1 and s == 0  # the point of the smaller old key


def test_the_merge_does_not_depend_on_the_order_of_the_voxels(H):
    calls, D, first = R.collapse(257)
    h = K.host_map(H, calls)
    shuffled = H(K.LEAF)
    keys = list(h.voxels)
    for k in np.random.default_rng(1).permutation(len(keys)).tolist():
        shuffled.voxels[keys[k]] = h.voxels[keys[k]]
    h.reproject(D, first), shuffled.reproject(D, first)
    assert h.size() == 1 and R.state(h) == R.state(shuffled)
    _, v, s = voxel(h, (0, -1, 2))
    assert v["count"] == 257 and v["frames"] == 2 and s == 0


# ---- clamp, drops ----------------------------------------------------------------------------------------------------------------
def test_sources_outside_the_corrections_take_the_nearest_entry(H):
    calls, D, first = R.clamp_below_and_above()
    h, dropped = R.reprojected_host(H, (calls, D, first))
    assert dropped == 0 and h.size() == 10
    pts, _ = h.get()
    for f, (was, _) in enumerate(calls):
        mine = pts[h.sources() == f]
        dy, dz = (0.5, 0.0) if f <= 2 else (0.0, -1.5)
        assert sorted(mine["y"].tolist()) == sorted((was["y"] + dy).tolist()) and sorted(mine["z"].tolist()) == sorted((was["z"] + dz).tolist())


def test_points_moved_out_of_the_index_range_drop_their_voxels(H):
    calls, D, first = R.drops()
    h = K.host_map(H, calls)
    assert h.size() == 4 and h.skipped == 0
    assert h.reproject(D, first) == R.DROPPED["drops"] == h.dropped and h.skipped == 0
    _, vox = h.get()
    assert vox["key"].tolist() == [K.key_of((7, 2, 0))] and h.sources().tolist() == [1]
    assert h.reproject(R.identity()) == 0 and h.dropped == 3  # a running count
    h.clear()
    assert h.dropped == 0


def test_no_corrections_are_refused(H):
    h = K.host_map(H, K.ties())
    before = R.state(h)
    with pytest.raises(ValueError):
        h.reproject(np.zeros((0, 16)))
    assert R.state(h) == before
    assert H(K.LEAF).reproject(R.identity()) == 0  # an empty map has nothing to move


# ---- where it agrees with a rebuild ----------------------------------------------------------------------------------------------
def test_single_point_voxels_reproject_to_the_map_rebuilt_from_the_moved_frames(H):
    frames, D = R.single_point_voxels()
    h = K.assert_nothing_skipped(H, frames)
    assert h.size() == 4097 and (h.get()[1]["count"] == 1).all()
    assert h.reproject(D) == 0
    rebuilt = H(K.LEAF)
    for (pts, f), d in zip(frames, D):
        moved = pts.copy()
        moved["x"] = (pts["x"].astype(np.float64) + d[3]).astype(np.float32)  # a translation along x, written without the definition
        rebuilt.insert(moved, f)
    assert rebuilt.skipped == 0 and 2000 < rebuilt.size() < 4000  # the translations force merges
    assert R.state(h) == R.state(rebuilt) and R.state(h, 2) == R.state(rebuilt, 2)
    assert h.get()[1]["frames"].max() >= 3


# ---- insertion goes on -----------------------------------------------------------------------------------------------------------
def test_an_insert_after_a_reprojection_applies_the_existing_voxel_rule(H):
    calls, D, first = R.merge_source_tie()
    h, _ = R.reprojected_host(H, (calls, D, first))
    with pytest.raises(ValueError):
        h.insert(calls[0][0], 1)  # the guard on the ordinals is the one of before: the last call had ordinal 2
    more = K.cloud([[0.375, 0.375, 0.375], [0.25, 0.0, 0.0], [9.0, 0.0, 0.0]], intensity=[6, 8, 1], first_index=40)
    h.insert(more[:1], 2)  # six against six: the voxel's point stays, last_frame is 2 already
    p, v, s = voxel(h, (0, 0, 0))
    assert s == 1 and (v["count"], v["frames"], v["last_frame"]) == (4, 3, 2)
    h.insert(more[1:], 3)
    p, v, s = voxel(h, (0, 0, 0))
    assert s == 3 and p["intensity"] == 8 and (v["count"], v["frames"], v["first_frame"], v["last_frame"]) == (5, 4, 0, 3)
    assert h.size() == 2 and h.sources().tolist() == [3, 3]


def test_every_case_for_the_device_is_what_it_says(H):
    for name, make in R.CASES.items():
        calls, D, first = make()
        assert D.shape[1] == 16 and D.dtype == np.float64 and D.shape[0] >= 1
        h, dropped = R.reprojected_host(H, (calls, D, first))
        assert dropped == R.DROPPED.get(name, 0), name
    for n in K.SIZES:
        h, dropped = R.reprojected_host(H, R.sized(n))
        assert dropped == 0 and h.size() <= n
    h, _ = R.reprojected_host(H, R.collapse())
    assert h.size() == 1 and h.get()[1]["count"][0] == 4097
    assert R.reprojected_host(H, R.CASES["skipping"]())[0].skipped == 7
