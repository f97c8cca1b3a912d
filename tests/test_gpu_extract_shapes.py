"""The extraction kernels at the shapes they branch on (tests/extract_cases.py).  The labelling kernel alone, through
lsa_selftest_labels, equals the plain reference greedy_labels and the oracle's SetKeyPointsLabels at every ring length where
its chunk size changes, at every window width, on scores that tie, chain and sit on the thresholds; whole frames at the
sizes the ring bucketing and the compaction branch on equal the oracle bit for bit."""
import numpy as np
import pytest

import extract_cases as EC

pytestmark = pytest.mark.gpu

CASES = EC.label_cases()
FRAMES = EC.frame_cases()


@pytest.fixture(scope="module")
def device_labels(gpu_ctx):
    out = {}
    for params, cases in EC.label_batches():  # at most 512 rings per launch
        out.update(EC.run_batch(gpu_ctx.selftest_labels, params, cases))
    return out


@pytest.fixture(scope="module")
def oracle_labels(O):
    ex, out = O.Extractor(), {}
    for params, cases in EC.label_batches():
        out.update(EC.run_batch(ex.label, params, cases))
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_labels_equal_the_reference_and_the_oracle(case, device_labels, oracle_labels):
    EC.assert_labels_equal(device_labels[case.name], EC.cached_reference(case), f"{case.name}: k_label against greedy_labels")
    EC.assert_labels_equal(device_labels[case.name], oracle_labels[case.name], f"{case.name}: k_label against the oracle")


def test_labelling_refuses_a_ring_of_8193_points(gpu_ctx, L):
    n = EC.MAX_RING_POINTS + 1
    z = np.zeros(n + 20, np.float32)
    with pytest.raises(L.LsaError) as e:
        gpu_ctx.selftest_labels([20, n], z, z, z, z, np.full(n + 20, 7, np.uint8))
    assert e.value.code == L.E_CAPACITY and "more than 8192 points on one laser ring" in str(e.value)
    case = CASES[0]
    EC.assert_labels_equal(gpu_ctx.selftest_labels(case.lens, *case.scores, case.valid, case.params), EC.cached_reference(case), "after the refusal")


def fixed_resolution(gpu_ctx, O):
    ex = O.Extractor()
    ex.azimuthal_resolution = gpu_ctx.azimuthal_resolution = EC.AZIMUTHAL_RESOLUTION
    return ex


@pytest.mark.parametrize("fc", FRAMES, ids=lambda f: f.name)
def test_whole_frames_equal_the_oracle(fc, gpu_ctx, O, L):
    counts = EC.assert_extraction_equal(gpu_ctx, fixed_resolution(gpu_ctx, O), O, L, fc.frame(), fc.params())
    if max(n for _, n in fc.rings) >= 2 * fc.W + 1:
        assert counts[0] > 0 and counts[2] > 0
    if fc.name == "rings_0_and_511":
        assert gpu_ctx.nb_laser_rings() == 512


def test_a_refused_frame_changes_no_keypoint_set(gpu_ctx, O, L):
    """A ring of 8193 points is refused.  The rule (include/lidarslam_amd.h, lsa_extract_keypoints): a refused frame
    changes neither keypoint set, so the next frame's previous keypoints are those of the last frame that was extracted."""
    ex = fixed_resolution(gpu_ctx, O)
    first, second = EC.scene_frame([(0, 3000), (1, 2049)]), EC.scene_frame([(0, 4097), (1, 1000)])
    EC.assert_extraction_equal(gpu_ctx, ex, O, L, first)
    want = [gpu_ctx.keypoints(L.SET_RAW_CURRENT, k) for k in range(3)]
    before = [gpu_ctx.keypoints(L.SET_RAW_PREVIOUS, k) for k in range(3)]
    assert all(a.size for a in want)
    gpu_ctx.upload_frame(EC.scene_frame([(0, EC.MAX_RING_POINTS + 1)]))
    with pytest.raises(L.LsaError) as e:
        gpu_ctx.extract_keypoints()
    assert e.value.code == L.E_CAPACITY and "more than 8192 points on one laser ring" in str(e.value)
    for k in range(3):
        assert gpu_ctx.keypoints(L.SET_RAW_CURRENT, k).tobytes() == want[k].tobytes()
        assert gpu_ctx.keypoints(L.SET_RAW_PREVIOUS, k).tobytes() == before[k].tobytes()
    EC.assert_extraction_equal(gpu_ctx, ex, O, L, second)
    for k in range(3):
        assert gpu_ctx.keypoints(L.SET_RAW_PREVIOUS, k).tobytes() == want[k].tobytes()


@pytest.mark.parametrize("mask", [0, 2, 5])
def test_kept_keypoint_types_on_a_ring_of_8192_points(mask, gpu_ctx, O, L):
    """the compaction's packed prefix sums at eight points per thread, and the time range over the kept types only"""
    ex = fixed_resolution(gpu_ctx, O)
    pts = EC.scene_frame([(0, EC.MAX_RING_POINTS), (1, 1025)])
    try:
        assert L.lib().lsa_set_keypoint_types(gpu_ctx.h, mask) == 0
        EC.assert_extraction_equal(gpu_ctx, ex, O, L, pts, mask=mask)
        gpu_ctx.reset_working_keypoints()
        t0, t1 = gpu_ctx.working_time_range()
        times = np.concatenate([ex.keypoints(k)["time"] for k in range(3) if (mask >> k) & 1] or [np.zeros(0)])
        if times.size:
            assert (t0, t1) == (times.min(), times.max())
        else:
            assert t0 > t1  # the reference's untouched initial values
    finally:
        assert L.lib().lsa_set_keypoint_types(gpu_ctx.h, 7) == 0
