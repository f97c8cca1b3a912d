"""The dense map's re-projection on the device (lsa_dense_map_reproject in lidarslam_amd/csrc/lsa_dense_reproject.hip,
lsa_dense_map_get_sources in lsa_dense_export.hip) against DenseMapHost.reproject, byte for byte on points, voxel records and sources, at
min_frames 1 and 2: every case of tests/dense_reproject_cases.py, sizes, contention on one slot, growth, long probe sequences,
rotations, refusals, insertion afterwards; and the pipeline under "DenseMapOnTrajectory"."""
import numpy as np
import pytest

import dense_map_cases as K
import dense_reproject_cases as R

pytestmark = pytest.mark.gpu


def same(device, host):
    """points, records and sources of the device map (or of (points, records, sources)) are the host's; returns the voxels"""
    for m in (1, 2):
        (dp, dv), ds = (device.get(m), device.sources(m)) if hasattr(device, "get") else (device(m)[:2], device(m)[2])
        hp, hv = host.get(m)
        assert dv.tobytes() == hv.tobytes(), (m, len(dv), len(hv))
        assert dp.tobytes() == hp.tobytes(), m
        assert ds.dtype == np.int32 and ds.tobytes() == host.sources(m).tobytes(), m
    return host.size()


def both(L, ctx, case, leaf=K.LEAF, **params):
    """the case's calls into a device map and the host statement, both re-projected -> (device, host)"""
    calls, D, first = case
    d = L.DenseMap(ctx, leaf, **params)
    h = L.DenseMapHost(leaf)
    for pts, frame in calls:
        d.insert_points(pts, frame)
        h.insert(pts, frame)
    same(d, h)  # the sources of the insertions themselves
    assert d.reproject(D, first) == h.reproject(D, first)
    return d, h


# ---- 1. the table alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_every_case_of_the_definition(L, gpu_ctx, name):
    d, h = both(L, gpu_ctx, R.CASES[name]())
    assert same(d, h) == d.size() and d.get_param("Dropped") == h.dropped == R.DROPPED.get(name, 0) and d.skipped() == h.skipped
    assert d.get_param("Reprojections") == 1 and d.get_param("ReprojectSeconds") > 0
    d.close()


@pytest.mark.parametrize("n", K.SIZES)
def test_sizes_under_a_translation_per_frame(L, gpu_ctx, n):
    d, h = both(L, gpu_ctx, R.sized(n))
    assert same(d, h) == d.size() <= n
    d.close()


def test_thousands_of_voxels_into_one_slot(L, gpu_ctx):
    d, h = both(L, gpu_ctx, R.collapse())
    assert same(d, h) == 1 == d.size()
    _, vox = d.get()
    assert vox["count"][0] == 4097 and vox["frames"][0] == 2
    d.close()


def test_sources_survive_growth_and_the_capacity_stays(L, gpu_ctx):
    calls = K.growth_calls()
    d, h = both(L, gpu_ctx, (calls, R.per_frame_translations(5), 0), InitialCapacity=64)
    assert d.get_param("Rehashes") >= 3
    capacity = d.get_param("Capacity")
    assert same(d, h) == d.size() < K.BATCH and capacity >= 2 * K.BATCH
    assert d.bytes() >= 68 * capacity
    # a second one, with first_frame in the middle, and an insertion behind it: the bound of the occupied slots is exact
    assert d.reproject(R.per_frame_translations(3), 2) == h.reproject(R.per_frame_translations(3), 2)
    more = K.distinct_voxels(4097, seed=77)
    d.insert_points(more, 4), h.insert(more, 4)
    assert same(d, h) == d.size() and d.get_param("Capacity") == capacity and d.get_param("Reprojections") == 2
    d.close()


def test_probe_stress_changes_nothing(L, gpu_ctx):
    d, h = both(L, gpu_ctx, (K.stress_calls(), R.per_frame_translations(2), 0), InitialCapacity=64, ProbeStress=1)
    assert same(d, h) == d.size() <= 2048
    d.close()


def test_a_small_rotation_narrows_to_float_as_numpy_does(L, gpu_ctx):
    leaf = 0.2
    calls = []
    for f in range(2):
        pts, _ = L.synth_frame(16, 1000, f)
        gpu_ctx.upload_frame(pts)
        n = gpu_ctx.L.lsa_frame_size(gpu_ctx.h)
        world = np.zeros(n, L.POINT_DTYPE)
        assert gpu_ctx.L.lsa_transform_frame_at(gpu_ctx.h, 0, L.ptr(L.pose16(L.synth_pose(f))), None, 0.0, 0.0, 0.0, L.ptr(world), n) == n
        calls.append((world, f))
    D = np.concatenate([R.small_rotation(0), R.small_rotation(1)])
    d, h = both(L, gpu_ctx, (calls, D, 0), leaf=leaf)
    assert same(d, h) > 5000 and h.dropped == 0
    # the host's move is the definition's, written once more here: every point the device kept is a moved point of its frame
    moved = {p.tobytes() for f, (world, _) in enumerate(calls) for p in R.move(world, D[f])}
    assert all(p.tobytes() in moved for p in d.get()[0])
    d.close()


def test_refusals_leave_the_bytes_and_a_further_insertion_follows_the_host(L, gpu_ctx):
    calls, D, first = R.merge_source_tie()
    d = L.DenseMap(gpu_ctx, K.LEAF)
    h = K.host_map(L.DenseMapHost, calls)
    for pts, frame in calls:
        d.insert_points(pts, frame)
    capacity = d.get_param("Capacity")
    with pytest.raises(L.LsaError) as e:
        d.reproject(np.zeros((0, 16)))
    assert e.value.code == L.E_ARG
    assert L.lib().lsa_dense_map_reproject(d.h, None, 0, 1, None) == L.E_ARG
    assert L.lib().lsa_dense_map_reproject(d.h, L.ptr(D), 0, -3, None) == L.E_ARG
    assert same(d, h) == 2 and d.get_param("Reprojections") == 0 and d.get_param("Capacity") == capacity
    assert d.reproject(D, first) == h.reproject(D, first) == 0
    assert same(d, h) == 1 == d.size() and d.get_param("Capacity") == capacity
    with pytest.raises(L.LsaError) as e:
        d.insert_points(calls[0][0], 1)  # the guard on the ordinals is unchanged
    assert e.value.code == L.E_ARG
    more = K.cloud([[0.375, 0.375, 0.375], [0.25, 0.0, 0.0], [9.0, 0.0, 0.0]], intensity=[6, 8, 1], first_index=40)
    for pts, frame in ((more[:1], 2), (more[1:], 3)):
        d.insert_points(pts, frame), h.insert(pts, frame)
        same(d, h)
    assert d.size() == 2 and d.sources().tolist() == [3, 3]
    d.clear()
    assert d.size() == 0 and d.get_param("Dropped") == 0 and d.sources().size == 0 and d.reproject(D, first) == 0
    d.close()


def test_pose_corrections_are_new_times_the_inverse_of_old(L):
    old = np.stack([L.synth_pose(f) for f in range(6)])
    new = old.copy()
    new[:, 0, 3] += 0.01 * np.arange(6)
    new[3:] = np.stack([R.small_rotation(f).reshape(4, 4) @ old[f] for f in range(3, 6)])
    D = L.pose_corrections(old, new)
    assert D.shape == (6, 16) and D.dtype == np.float64
    # products and sums of a few doubles of unit scale (rotation entries, translations of metres): 1e-12 is thousands of ulps
    assert np.abs(D.reshape(-1, 4, 4) - new @ np.linalg.inv(old)).max() < 1e-12
    assert (D[:, 12:] == [0, 0, 0, 1]).all()


# ---- 2. the pipeline ---------------------------------------------------------------------------------------------------------
PIPE_LEAF = 0.2


@pytest.fixture(scope="module")
def drive(L):
    return [L.synth_frame(16, 1000, f) for f in range(10)]


def mapped(L, drive, frames, on_trajectory, **params):
    s = L.Slam(0, EgoMotion=3, DenseMap=1, DenseMapLeafSize=PIPE_LEAF, DenseMapOnTrajectory=on_trajectory, **params)
    h = L.DenseMapHost(PIPE_LEAF)
    for f in range(frames):
        s.add_frame(*drive[f], f)
        h.insert(s.registered_frame().copy(), f)
    return s, h


def pipeline_state(L, s):
    return lambda m: (*L.dense_map(s, m), L.dense_map_sources(s, m))


def shifted(P):
    P2 = P.copy().reshape(-1, 4, 4)
    P2[:, 0, 3] += 0.01 * np.arange(P2.shape[0])
    return P2


def test_an_applied_trajectory_reprojects_the_map_and_mapping_goes_on(L, drive):
    s, h = mapped(L, drive, 6, 1, LoggingTimeout=-1)
    assert s.get_param("DenseMapOnTrajectory") == 1
    assert same(pipeline_state(L, s), h) > 5000
    P, t, _ = s.trajectory()
    P2 = shifted(P)
    s.set_trajectory(P2, t)
    assert h.reproject(L.pose_corrections(P, P2)) == s.get_param("DenseMapDropped") == 0
    assert same(pipeline_state(L, s), h) == L.dense_map_size(s) > 5000
    assert s.get_param("DenseMapClears") == 0 and s.get_param("DenseMapReprojections") == 1 and s.get_param("DenseMapFrames") == 6
    for f in range(6, 9):  # ordinals 6, 7, 8
        s.add_frame(*drive[f], f)
        h.insert(s.registered_frame().copy(), f)
    same(pipeline_state(L, s), h)
    assert set(np.unique(L.dense_map_sources(s))) <= set(range(9)) and L.dense_map(s)[1]["last_frame"].max() == 8
    # what clears under 0 clears under 1
    L.clear_dense_map(s)
    assert L.dense_map_size(s) == 0 and s.get_param("DenseMapClears") == 1 and s.get_param("DenseMapFrames") == 0
    s.close()


def test_without_the_parameter_an_applied_trajectory_clears_as_before(L, drive):
    s, _ = mapped(L, drive, 6, 0, LoggingTimeout=-1)
    assert s.get_param("DenseMapOnTrajectory") == 0 and L.dense_map_size(s) > 5000
    P, t, _ = s.trajectory()
    s.set_trajectory(shifted(P), t)
    assert L.dense_map_size(s) == 0 and s.get_param("DenseMapClears") == 1 and s.get_param("DenseMapReprojections") == 0
    assert L.dense_map_sources(s).size == 0
    h = L.DenseMapHost(PIPE_LEAF)
    for i, f in enumerate(range(6, 8)):  # the ordinals start again
        s.add_frame(*drive[f], f)
        h.insert(s.registered_frame().copy(), i)
    same(pipeline_state(L, s), h)
    with pytest.raises(KeyError):
        s.set_param("DenseMapOnTrajectory", 2)
    s.close()


def test_ordinals_that_left_the_log_take_the_oldest_logged_correction(L, drive):
    s, h = mapped(L, drive, 8, 1, LoggingTimeout=0.35)  # three and a half frame periods
    P, t, _ = s.trajectory()
    logged = P.shape[0]
    assert 2 <= logged < 8 and s.get_param("DenseMapFrames") == 8
    P2 = shifted(P)
    P2[:, 1, 3] -= 0.25  # the oldest logged pose moves too: the ordinals before it go with it
    s.set_trajectory(P2, t)
    assert h.reproject(L.pose_corrections(P, P2), 8 - logged) == 0
    assert same(pipeline_state(L, s), h) > 5000 and s.get_param("DenseMapReprojections") == 1 and s.get_param("DenseMapClears") == 0
    s.close()


def test_an_applied_optimization_keeps_the_map_under_the_poses_it_applied(L, drive):
    s, h = mapped(L, drive, 6, 1, LoggingTimeout=-1)
    P, t, _ = s.trajectory()
    relative = np.linalg.inv(P[0]) @ P[5]
    relative[0, 3] += 0.05  # a loop edge that disagrees with the odometry by five centimetres
    got, times, res = s.optimize_trajectory([(0, 5, relative, np.eye(6) * 1e4)], apply=True)
    assert np.abs(got - P).max() > 1e-3 and (times == t).all()
    assert (s.trajectory()[0] == got).all()
    h.reproject(L.pose_corrections(P, got))
    assert same(pipeline_state(L, s), h) > 5000 and s.get_param("DenseMapReprojections") == 1 and s.get_param("DenseMapClears") == 0
    s.close()
