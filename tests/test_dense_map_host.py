"""DenseMapHost (lidarslam_amd/_dense_map.py), the statement the device's dense map is held to: its properties, on the cases
of tests/dense_map_cases.py.  No GPU."""
import numpy as np
import pytest

import dense_map_cases as K


@pytest.fixture(scope="module")
def H(L):
    return L.DenseMapHost


def test_the_record_is_the_c_struct(L):
    d = L.dense_voxel_dtype
    assert d.itemsize == 24 and [d.fields[n][1] for n in ("key", "count", "frames", "first_frame", "last_frame")] == [0, 8, 12, 16, 20]


def test_negative_coordinates_floor(H):
    calls, indices = K.negative_coordinates()
    h = K.assert_nothing_skipped(H, calls)
    pts, vox = h.get()
    assert sorted(vox["key"].tolist()) == sorted({K.key_of(i) for i in indices}) and len(vox) == 4
    # -0.0 and the z = -0.0 point share voxel 0 with each other, not with -0.125
    zero = vox[vox["key"] == K.key_of((0, 0, 0))][0]
    assert zero["count"] == 2 and pts[vox["key"] == K.key_of((0, 0, 0))]["intensity"][0] == 5
    assert vox[vox["key"] == K.key_of((-1, 0, 0))]["count"][0] == 1


def test_points_on_faces_belong_to_the_voxel_above(H):
    calls, indices = K.faces()
    h = K.assert_nothing_skipped(H, calls)
    _, vox = h.get()
    assert vox["key"].tolist() == sorted(K.key_of(i) for i in indices) and (vox["count"] == 1).all()
    assert (np.diff(vox["key"].astype(np.int64)) > 0).all()  # ascending key: z-major


def test_ties_within_a_call_and_across_calls(H):
    (a, _), (b, _) = calls = K.ties()
    h = K.assert_nothing_skipped(H, calls[:1])
    pts, vox = h.get()
    assert pts[0].tobytes() == a[1].tobytes() and vox[0]["count"] == 4  # of the two nines, the lower index
    h.insert(b, 1)
    pts, vox = h.get()
    assert pts[0].tobytes() == a[1].tobytes()  # nine against nine: the earlier frame keeps it
    assert pts[1].tobytes() == b[3].tobytes()  # five against four: replaced
    assert vox["count"].tolist() == [7, 2] and vox["frames"].tolist() == [2, 2]
    assert vox["first_frame"].tolist() == [0, 0] and vox["last_frame"].tolist() == [1, 1]


def test_a_nan_intensity_loses_to_every_number(H):
    (a, _), (b, _) = calls = K.nan_intensity()
    h = K.assert_nothing_skipped(H, calls[:1])
    pts, _ = h.get()
    assert pts[0].tobytes() == a[1].tobytes()  # -inf beats the NaNs around it
    assert pts[1].tobytes() == a[3].tobytes()  # NaNs alone: the lowest index
    h.insert(b, 3)
    pts, vox = h.get()
    assert pts[0].tobytes() == a[1].tobytes()  # a later NaN replaces nothing
    assert pts[1].tobytes() == b[0].tobytes()  # any number replaces a NaN
    assert pts[2].tobytes() == a[5].tobytes()
    assert vox["last_frame"].tolist() == [3, 3, 3] and vox["frames"].tolist() == [2, 2, 2]


def test_minus_zero_ranks_below_plus_zero(H):
    (a, _), (b, _) = calls = K.signed_zero()
    h = K.assert_nothing_skipped(H, calls[:1])
    pts, _ = h.get()
    assert pts[0].tobytes() == a[1].tobytes()  # +0.0 behind -0.0 in the call: it wins all the same
    h.insert(b, 1)
    pts, vox = h.get()
    assert pts[0].tobytes() == a[1].tobytes()  # -0.0 of a later frame against +0.0: kept
    assert pts[1].tobytes() == b[0].tobytes()  # +0.0 against -0.0: strictly greater, replaced
    assert pts[2].tobytes() == a[3].tobytes()  # -0.0 against +0.0: kept
    assert np.signbit(pts["intensity"]).tolist() == [False, False, False] and vox["count"].tolist() == [3, 2, 2]


def test_non_finite_and_out_of_range_points_are_skipped(H):
    calls, skipped, indices = K.skipping()
    h = K.host_map(H, calls)
    assert h.skipped == skipped
    _, vox = h.get()
    assert vox["key"].tolist() == sorted(K.key_of(i) for i in indices)
    assert K.key_of(((1 << 20) - 1,) * 3) < 1 << 63  # every key leaves bit 63 free


def test_the_same_ordinal_twice_counts_one_frame(H):
    calls = K.same_ordinal_twice()
    h = K.assert_nothing_skipped(H, calls)
    pts, vox = h.get()
    assert vox["count"].tolist() == [4, 1, 1] and vox["frames"].tolist() == [2, 1, 1]
    assert vox["first_frame"].tolist() == [4, 4, 4] and vox["last_frame"].tolist() == [6, 4, 4]
    assert pts[0].tobytes() == calls[1][0][0].tobytes()
    with pytest.raises(ValueError):
        h.insert(calls[0][0], 5)  # ordinals must not decrease


def test_min_frames_keeps_the_wall_and_drops_the_mover(H):
    calls, wall = K.wall_and_mover()
    h = K.assert_nothing_skipped(H, calls)
    _, everything = h.get()
    _, kept = h.get(3)
    assert len(everything) == wall + len(calls) and len(kept) == wall
    assert (kept["frames"] == len(calls)).all() and (kept["count"] == len(calls)).all()
    assert (everything["frames"][~np.isin(everything["key"], kept["key"])] == 1).all()


@pytest.mark.parametrize("order", ["interleaved", "reversed"])
def test_the_map_does_not_depend_on_the_arrival_order_but_for_ties(L, H, order):
    """the same multiset of points in another order: same voxel records; the point kept is the first of the largest intensity in
    THAT order, which a direct walk over the call confirms"""
    base, other = K.runs("contiguous"), K.runs(order)
    hb, ho = K.assert_nothing_skipped(H, [(base, 0)]), K.assert_nothing_skipped(H, [(other, 0)])
    assert hb.get()[1].tobytes() == ho.get()[1].tobytes()
    pts, vox = ho.get()
    keys, ok = L.dense_voxel_keys(other, K.LEAF)
    assert ok.all()
    for j in (0, len(vox) // 2, len(vox) - 1, int(np.argmax(vox["count"]))):
        mine = np.flatnonzero(keys == vox["key"][j])
        best = mine[np.flatnonzero(other["intensity"][mine] == other["intensity"][mine].max())[0]]
        assert pts[j].tobytes() == other[best].tobytes() and vox["count"][j] == mine.size
    assert sorted(np.unique(vox["count"]).tolist()) == sorted(set(K.RUNS))


def test_the_cases_for_the_device_skip_nothing(H):
    for n in K.SIZES:
        h = K.assert_nothing_skipped(H, [(K.distinct_voxels(n), 0)])
        assert h.size() == n
    assert K.assert_nothing_skipped(H, [(K.one_voxel(4097), 0)]).size() == 1
    assert K.assert_nothing_skipped(H, K.growth_calls()).size() == K.BATCH
    assert K.assert_nothing_skipped(H, K.stress_calls()).size() == 2048
    for name, make in K.PROPERTY_CASES.items():
        if name != "skipping":
            K.assert_nothing_skipped(H, make())
