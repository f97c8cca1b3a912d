"""The reference the keypoint labelling is held to (extract_cases.greedy_labels) against the oracle's own
SetKeyPointsLabels on every case of tests/extract_cases.py, the conditions that keep those cases from being vacuous, and
the scene generator's frames.  No GPU: tests/test_gpu_extract_shapes.py holds the kernels to the same cases."""
import numpy as np
import pytest

import extract_cases as EC

CASES = EC.label_cases()
FRAMES = EC.frame_cases()


def test_greedy_labels_on_a_ring_worked_by_hand(L):
    """NeighborWidth 1, twelve points: windows 0 (depth gap), 1 (angle), 0 (saliency), 1 (intensity gap), 4 (planes).
    Depth gap 1 >= 0.0225 at 2 and 9 (window 0: both, nothing else cleared).  Angle 0.9 at 4, 5, 6: the equal scores go by
    ascending index, 4 wins and clears 3-5, then 6.  Intensity gap 60 at 0 and 1 and 70 at 10 and 11: 10 (the smaller index of
    the larger score) clears 9-11, then 0 clears 0-1.  Planes: 0.25 everywhere else, walked from the back: 11 clears 7-11, 3
    clears 0-7 (4, 5, 6 are no candidates, and 6 < 7 so 7 fell to 11).  Blobs: 0, 3, 6, 9."""
    n = 12
    angle = np.full(n, 0.25, np.float32)
    angle[4:7] = 0.9
    gap, sal, inten = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    gap[[2, 9]] = 1.0
    inten[[0, 1]], inten[[10, 11]] = 60.0, 70.0
    label, after = EC.greedy_labels((angle, gap, sal, inten), np.full(n, 7, np.uint8), 1, EC.thresholds(L.ExtractParams(neighbor_width=1)))
    edges, planes, blobs = (np.flatnonzero(label & (1 << k)).tolist() for k in range(3))
    assert (edges, planes, blobs) == ([0, 2, 4, 6, 9, 10], [3, 11], [0, 3, 6, 9])
    # validity afterwards: cleared in the windows, set back on the labelled points themselves
    assert np.flatnonzero(after & 1).tolist() == [0, 2, 4, 6, 8, 9, 10]  # 8 alone was in no window
    assert np.flatnonzero(after & 2).tolist() == [3, 11]
    assert np.all(after & 4)


def test_the_cases_cover_what_the_kernel_branches_on():
    by = {(c.lens[0], c.W, c.pattern) for c in CASES if c.lens.size == 1}
    for n in [8, 9, 10, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192]:
        assert all((n, 4, p) in by for p in EC.PATTERNS), n
    for W in (1, 5, 8):
        assert all((n, W, p) in by for n in (1025, 2049, 4097, 8192) for p in EC.PATTERNS), W
    assert {EC.chunk_size(c.lens[0]) for c in CASES if c.lens.size == 1} == {1, 2, 4, 8}
    assert any(c.lens[0] % EC.chunk_size(c.lens[0]) for c in CASES if c.lens[0] > 4096)  # a ring that is no multiple of PER
    multi = [c for c in CASES if c.lens.size > 1]
    assert len(multi) == 1 and multi[0].lens.size == 512 and multi[0].lens[511] > 0 and multi[0].lens[2] == 0
    assert {EC.chunk_size(n) for n in multi[0].lens if n >= 9} == {1, 2, 4, 8} and any(0 < n < 9 for n in multi[0].lens)
    assert float(EC.F_BELOW_1E6) < 1e-6 <= float(EC.F_ABOVE_1E6) and np.nextafter(EC.F_BELOW_1E6, np.float32(1)) == EC.F_ABOVE_1E6


@pytest.fixture(scope="module")
def oracle_labels(O):
    ex, out = O.Extractor(), {}
    for params, cases in EC.label_batches():
        out.update(EC.run_batch(ex.label, params, cases))
    return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_greedy_labels_equal_the_oracle(case, oracle_labels):
    EC.assert_labels_equal(EC.cached_reference(case), oracle_labels[case.name], f"{case.name}: greedy_labels against the oracle")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_no_case_is_vacuous(case):
    assert not EC.vacuity_problems(case)


@pytest.mark.parametrize("fc", FRAMES, ids=lambda f: f.name)
def test_scene_frames_yield_keypoints_on_every_ring(fc, O):
    """By the oracle alone: every ring of at least 2W+1 points yields an edge and a plane keypoint.  (At NeighborWidth 1 the
    reference fits its two lines to one point each: there is no direction, the sin angle is 0 and no point is ever a plane
    -- edges only.)"""
    pts = fc.frame()
    assert pts.size == sum(n for _, n in fc.rings)
    firing = pts if not fc.by_ring else pts[np.argsort(pts["time"], kind="stable")]
    assert np.all(np.diff(firing["time"]) > 0)
    assert np.unique(pts["intensity"]).size <= 3
    ex = O.Extractor()
    ex.azimuthal_resolution = EC.AZIMUTHAL_RESOLUTION
    ex.compute(pts, fc.params())
    edge, plane = ex.debug(4), ex.debug(5)
    for ring, n in fc.rings:
        on = pts["laser_id"] == ring
        assert np.count_nonzero(on) == n
        if n >= 2 * fc.W + 1:
            assert edge[on].sum() > 0, (ring, n)
            assert plane[on].sum() > 0 or fc.W == 1, (ring, n)
        else:
            assert edge[on].sum() == 0 and plane[on].sum() == 0
