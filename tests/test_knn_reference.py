"""The brute-force kNN reference of tests/knn_cases.py has to be trusted before the search kernels are held to it
(tests/test_gpu_knn_routes.py): exact against integer arithmetic where the data allow it, within float32 rounding of a
float64 brute force elsewhere, and every case keeps what it declares of itself.  No GPU."""
import numpy as np
import pytest

import knn_cases as K

ANCHORED = {c.name for c in K.CASES if np.array_equal(K.xyz32(c.target)[:2], K.ANCHORS.astype(np.float32))}


@pytest.mark.parametrize("case", [c for c in K.CASES if c.lattice], ids=lambda c: c.name)
def test_lattice_reference_equals_integer_brute_force(case):
    """every coordinate is a multiple of 0.5 below 16: products and sums are exact in float32, so lists and order must be
    those of int64 arithmetic on the doubled coordinates"""
    idx, d2 = K.reference(case)
    ii, d4 = K.brute_knn_int(K.xyz32(case.target), K.xyz32(case.queries), case.k)
    assert np.array_equal(idx, ii)
    assert np.array_equal(d2.astype(np.float64) * 4.0, d4.astype(np.float64))
    # the case is about ties: the k-th place falls inside a group of equal distances for a good share of the queries
    full = K.brute_knn_int(K.xyz32(case.target), K.xyz32(case.queries), case.k + 1)[1]
    assert (full[:, case.k - 1] == full[:, case.k]).mean() > 0.25


@pytest.mark.parametrize("case", [c for c in K.CASES if not c.lattice], ids=lambda c: c.name)
def test_float_reference_is_within_rounding_of_float64(case, O):
    """k-th float32 distance within 2 ulp of the float64 one; the neighbour SET equals the float64 set wherever the float64
    gap behind the k-th place is wider than that"""
    t, q = K.xyz32(case.target), K.world_queries(case, O)
    idx, d2 = K.reference(case, O)
    i64, d64 = K.brute_knn_f64(t, q, case.k)
    kk = idx.shape[1]
    assert kk == min(case.k, t.shape[0])
    if kk == 0:
        return
    kth32, kth64 = d2[:, kk - 1].astype(np.float64), d64[:, kk - 1]
    tol = 2.0 * np.spacing(d2[:, kk - 1]).astype(np.float64)  # 2 ulp of the float32 value
    assert np.all(np.abs(kth32 - kth64) <= tol), np.abs(kth32 - kth64).max()
    if d64.shape[1] > kk:
        clear = d64[:, kk] - kth64 > tol
        assert clear.any() or case.name.startswith("degenerate_identical")
        same = np.array([set(a) == set(b) for a, b in zip(idx[clear], i64[clear][:, :kk])])
        assert same.all()
    # ascending by (distance bits, index), no index twice
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    assert np.all(key[:, 1:] > key[:, :-1])


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_cases_keep_what_they_declare(case, O):
    m, nq = case.target.size, case.queries.size
    assert m <= 16384 and nq <= 2048 and 1 <= case.k <= K.KNN_MAX
    far = K.beyond_rejection(case, O)
    if case.name.startswith("far_"):
        assert m >= case.k and case.ktype != K.EDGE
        assert 0.0 < far.mean() < 1.0  # neither branch of the far assertion is vacuous
    else:
        assert not far.any()
    if case.settled_within is not None:
        assert np.all(K.reference(case, O)[1][:, case.k - 1] < case.settled_within)
    lv = K.grid_levels(K.xyz32(case.target), case.cell)
    grows = case.tags.get("grows")
    assert case.anchored == (case.name in ANCHORED)
    if case.anchored:
        assert [c for c, _ in lv] == [1.0, 4.0, 16.0]  # the neat radii the derivations use
    if grows == "level0":
        assert lv[0][0] > case.cell and lv[1][0] == 4 * lv[0][0] and lv[2][0] == 4 * lv[1][0]
    if grows == "flat":
        assert lv[0][0] > case.cell and lv[1][0] == np.float32(4 * lv[0][0]) and lv[2][0] > 4.5 * lv[1][0]
    if grows == "flat2":
        assert lv[0][0] == case.cell and lv[1][0] > 4.5 * lv[0][0] and lv[2][0] > 4.5 * lv[1][0]
    if case.name.startswith("covered") or case.name.startswith("degenerate_identical"):
        assert all(d <= 2 for d in lv[0][1])  # any 3^3 block covers the grid
    if case.name.startswith("degenerate_line"):
        assert sorted(lv[0][1])[:2] == [1, 1]
    if case.name.startswith("degenerate_plane"):
        assert lv[0][1][2] == 1


def test_anchored_sites_sit_where_the_derivations_put_them():
    """the numbers the routed cases' comments use: which block of the site holds how many points (plain counting in the
    documented boxes, not the search's block choice)"""
    def inside(case, lo, hi):
        t = K.xyz32(case.target).astype(np.float64)
        return int(np.all((t >= lo) & (t < hi), axis=1).sum())

    shells = [(71, 74), (70, 75), (68, 80), (64, 84), (48, 96), (32, 112), (16, 128)]
    for sh2, first, name in ((1, 0, "second_scan_sh1_edge10"), (2, 0, "second_scan_sh2_plane5"), (3, 2, "second_scan_sh3_edge16"), (4, 3, "second_scan_sh4_plane8"),
                             (5, 4, "second_scan_sh5_blob10"), (6, 5, "second_scan_sh6_plane16")):
        c = K.BY_NAME[name]
        counts = [inside(c, *s) for s in shells]
        need = 3 * c.k if first == 0 else c.k
        assert counts[first] == need and (first == 0 or counts[first - 1] == 0), (name, counts)
        assert counts[sh2] == need + (c.k // 2 if sh2 >= 2 else 0), (name, counts)  # the decoys: outside the first block, inside the second
        d2 = K.reference(c)[1]
        # after the first scan the k-th best is the cluster's k-th: beyond what the first block proves, inside what sh2 does
        t = K.xyz32(c.target)[2:2 + need].astype(np.float64)
        kth = np.sort(((K.xyz32(c.queries).astype(np.float64)[:, None, :] - t[None]) ** 2).sum(2), axis=1)[:, c.k - 1]
        assert np.all(kth > K.PROVEN[first] ** 2) and np.all(kth < K.PROVEN[sh2] ** 2) and np.all(kth > K.PROVEN[sh2 - 1] ** 2)
        assert np.all(d2[:, c.k - 1] <= kth + 1e-3)
    for name in ("heavy_first_192_plane5", "heavy_first_193_plane5", "heavy_second_plane16"):
        c = K.BY_NAME[name]
        counts = [inside(c, *s) for s in shells]
        if "first" in name:
            assert (counts[0] > K.HEAVY) == ("all_heavy" in c.routes) and counts[0] in (K.HEAVY, K.HEAVY + 1)
        else:
            assert counts[0] == 3 * c.k <= K.HEAVY < counts[1]
    for c in K.CASES:
        if c.name.startswith("far_later"):
            d = float(c.mp.max_neighbors_distance)
            far_d2 = np.float32(d * d * 1.0001)
            s = next(i for i in range(7) if np.float32(K.PROVEN[i]) ** 2 > far_d2)
            assert s >= 3 and inside(c, *shells[s]) == 0  # the first shell to prove more holds nothing: rejected by its count


def test_every_compiled_list_length_and_k_is_selected():
    picked = {K.compiled_lengths(c.ktype, c.k) for c in K.CASES}
    assert picked == {(8, 5, 0), (10, 5, 0), (16, 5, 16), (16, 8, 16), (16, 16, 16)}
    assert {c.k for c in K.CASES if c.ktype == K.EDGE} >= {2, 8, 10, 16}
    assert {c.k for c in K.CASES if c.ktype == K.PLANE} >= {3, 5, 8, 16}
    assert any(c.ktype == K.BLOB for c in K.CASES) and any(c.ktype != K.BLOB for c in K.CASES)
    assert {c.queries.size for c in K.CASES} >= {1, 31, 32, 33}


def test_case_construction_is_deterministic():
    again = K.build_cases()
    assert [c.name for c in again] == [c.name for c in K.CASES]
    for a, b in zip(again, K.CASES):
        assert a.target.tobytes() == b.target.tobytes() and a.queries.tobytes() == b.queries.tobytes()
        assert bytes(a.mp) == bytes(b.mp) and a.routes == b.routes


def test_brute_force_orders_ties_by_index():
    t = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 0, 1], [0, 0, 0], [0, -1, 0]], np.float32)
    idx, d2 = K.brute_knn(t, np.zeros((1, 3), np.float32), 4)
    assert idx.tolist() == [[4, 0, 1, 2]] and d2.tolist() == [[0.0, 1.0, 1.0, 1.0]]
    idx, _ = K.brute_knn(t, np.zeros((1, 3), np.float32), 16)
    assert idx.tolist() == [[4, 0, 1, 2, 3, 5]]  # min(k, m)
