"""The argument the search's list keeping rests on (lsa_knn.h: key_min_f64 / key_max_f64, LaneList::order2, group_min): a
64-bit (distance bits, index) key at or below kKeyEmpty, read as a float64, is finite and never NaN, and the IEEE order of
such doubles is the unsigned order of their bits -- so v_min_f64 / v_max_f64 on the bits are the integer minimum and
maximum.  Checked with numpy's float64 on the boundary keys and on random ones; and the cases of tests/knn_list_cases.py
are held to what they claim and their float32 references to integer / float64 brute forces.  No GPU."""
import numpy as np
import pytest

import knn_cases as K
import knn_list_cases as C

INT_MAX = 0x7FFFFFFF
KEY_EMPTY = (0x7F800000 << 32) | INT_MAX
BOUNDARY_BITS = [0, 1, 0x000FFFFF, 0x00100000, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000]


def domain():
    keys = [(d << 32) | i for d in BOUNDARY_BITS for i in (0, 1, INT_MAX - 1)] + [KEY_EMPTY]
    rng = np.random.default_rng(5)
    rnd = (rng.integers(0, 0x7F800000, 4000, dtype=np.uint64, endpoint=True) << np.uint64(32)) | rng.integers(0, INT_MAX, 4000, dtype=np.uint64)
    # and keys that differ in the index alone, or in the lowest distance bit alone
    near = np.concatenate([rnd[:500] ^ np.uint64(1), rnd[:500] ^ (np.uint64(1) << np.uint64(32))])
    k = np.unique(np.concatenate([np.array(keys, np.uint64), rnd, near]))
    return k[k <= np.uint64(KEY_EMPTY)]


def test_keys_are_finite_doubles():
    k = domain()
    f = k.view(np.float64)
    assert np.all(np.isfinite(f)) and not np.signbit(f).any()
    # exponent field at most 0x7f8: the upper word is at most 0x7f800000
    assert int((k >> np.uint64(52)).max()) <= 0x7F8
    # the range the issue names: distance bits below 0x00100000 are f64 denormals (exponent field 0), distance 0 included
    den = (k >> np.uint64(32)) < np.uint64(0x00100000)
    assert den.any() and np.all((k[den] >> np.uint64(52)) == 0) and np.all((k[~den] >> np.uint64(52)) > 0)


def test_float_order_is_unsigned_order():
    k = domain()  # ascending as unsigned, unique
    f = k.view(np.float64)
    assert np.all(f[1:] > f[:-1])
    rng = np.random.default_rng(6)
    a, b = rng.choice(k, 20000), rng.choice(k, 20000)
    # every boundary key against every other one too
    edge = np.array([(d << 32) | i for d in BOUNDARY_BITS for i in (0, 1, INT_MAX - 1)] + [KEY_EMPTY], np.uint64)
    a = np.concatenate([a, np.repeat(edge, edge.size)])
    b = np.concatenate([b, np.tile(edge, edge.size)])
    fa, fb = a.view(np.float64), b.view(np.float64)
    assert np.array_equal(fa < fb, a < b) and np.array_equal(fa == fb, a == b)
    # WHICH key minimum / maximum return, as bit patterns
    assert np.array_equal(np.minimum(fa, fb).view(np.uint64), np.minimum(a, b))
    assert np.array_equal(np.maximum(fa, fb).view(np.uint64), np.maximum(a, b))


def test_a_sorted_insertion_by_min_max_is_the_integer_one():
    """LaneList::sink as written in the kernel, on float64 views against uint64"""
    rng = np.random.default_rng(7)
    k = domain()
    for kmax in (5, 8, 10, 16):
        vi = np.full(kmax, KEY_EMPTY, np.uint64)
        vf = vi.view(np.float64).copy()
        for key in rng.choice(k, 200):
            if key < vi[kmax - 1]:
                vi[kmax - 1] = key
                vf[kmax - 1] = np.array([key], np.uint64).view(np.float64)[0]
                for s in range(kmax - 1, 0, -1):
                    lo, hi = min(vi[s - 1], vi[s]), max(vi[s - 1], vi[s])
                    vi[s - 1], vi[s] = lo, hi
                    flo, fhi = np.minimum(vf[s - 1], vf[s]), np.maximum(vf[s - 1], vf[s])
                    vf[s - 1], vf[s] = flo, fhi
            assert np.array_equal(vf.view(np.uint64), vi)
        assert np.all(vi[1:] >= vi[:-1])


# ------------------------------------------------------------------------------------------------ the GPU cases
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_list_case_reference_is_within_rounding_of_float64(case):
    """as tests/test_knn_reference.py for the cases of knn_cases: the k-th float32 distance within rounding of the float64 one,
    the neighbour set the float64 set wherever the gap behind the k-th place is wider than that, lists strictly ascending.
    Rounding: three products and two sums at half an ulp of the result each (2.5 ulp), and three differences q - p that are
    not exact here (queries up to 2.5 cells from points of any magnitude): 2^-24 relative each, 2^-23 on the squares, at
    most 2 ulp of their sum -- 4.5 ulp of the float32 value."""
    t, q = K.xyz32(case.target), K.xyz32(case.queries)
    assert t.shape[0] <= 4096 and q.shape[0] <= 64
    idx, d2 = K.reference(case)
    i64, d64 = K.brute_knn_f64(t, q, case.k)
    kk = idx.shape[1]
    assert kk == min(case.k, t.shape[0]) and kk > 0
    kth32, kth64 = d2[:, kk - 1].astype(np.float64), d64[:, kk - 1]
    tol = 4.5 * np.spacing(d2[:, kk - 1]).astype(np.float64)
    assert np.all(np.abs(kth32 - kth64) <= tol)
    if d64.shape[1] > kk:
        clear = d64[:, kk] - kth64 > tol
        assert all(set(a) == set(b) for a, b in zip(idx[clear], i64[clear][:, :kk]))
    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    assert np.all(key[:, 1:] > key[:, :-1])
    if case.anchored:
        assert [c for c, _ in K.grid_levels(t, case.cell)] == [1.0, 4.0, 16.0]


@pytest.mark.parametrize("case", [c for c in C.CASES if c.name.startswith("zero_denormal")], ids=lambda c: c.name)
def test_zero_and_denormal_distances_are_what_the_case_says(case):
    idx, d2 = K.reference(case)
    b = d2.view(np.uint32)
    k = case.k
    # offsets squared: float32 denormals on both sides of 0x00100000, in the kernels' arithmetic
    ob = [int(C.kernel_d2([0, 0, 0], [o, 0, 0]).view(np.uint32)) for o in C.OFFSETS]
    assert 0 < ob[0] < ob[1] < 0x00100000 < ob[2] < 0x00800000 and ob[2] < 0x00100000 + 0x20000
    full, thin = [i for i in range(16) if i % 4 < 2], [i for i in range(16) if i % 4 >= 2]
    # full sites: the whole list at distance bits 0, the k lowest indices of the k + 3 copies in ascending order
    assert np.all(b[full] == 0) and np.all(np.diff(idx[full].astype(np.int64), axis=1) > 0)
    # thin sites: two zeros, then two keys each at the three denormal distances, ties in index order
    want = [0, 0] + [v for v in ob for _ in range(2)]
    n = min(k, 8)
    assert np.all(b[thin][:, :n] == np.array(want[:n], np.uint32))
    for row in idx[thin][:, :n]:
        assert all(row[j] < row[j + 1] for j in range(0, n - 1, 2))
    if k > 8:
        assert np.all(b[thin][:, 8] >= 0x00800000)


@pytest.mark.parametrize("case", [c for c in C.CASES if c.name.startswith("bound_")], ids=lambda c: c.name)
def test_bound_cases_put_the_pair_where_the_second_scan_decides(case):
    sh2, first, ub = case.tags["bound"]
    t, q = K.xyz32(case.target), K.xyz32(case.queries)[0]
    k, im, ix, ip = case.k, case.tags["mirror"], case.tags["beyond"], case.tags["kth"]
    d = np.array([C.kernel_d2(q, p) for p in t])
    # equal in float32 in the kernels' expression order, and exactly (all coordinates are multiples of 2^-17 below 2^7)
    assert d[im].view(np.uint32) == d[ip].view(np.uint32) == np.float32(ub).view(np.uint32) and im < ip
    assert d[ix] == np.nextafter(np.float32(ub), np.float32(np.inf))
    ti, qi = np.rint(t.astype(np.float64) * 2.0 ** 17).astype(np.int64), np.rint(q.astype(np.float64) * 2.0 ** 17).astype(np.int64)
    assert np.array_equal(ti, t.astype(np.float64) * 2.0 ** 17)
    e = ((ti - qi[None, :]) ** 2).sum(1)
    assert e[im] == e[ip] < e[ix]
    # the first block: holds P and exactly k - 1 nearer points (and, shell 0, 2k farther ones), neither M nor X
    lo, hi = C.FIRST_BLOCK[first]
    inside = np.all((t >= lo) & (t < hi), axis=1)
    assert inside[ip] and not inside[im] and not inside[ix]
    assert int(inside.sum()) == (3 * k if first == 0 else k) and int((inside & (e < e[ip])).sum()) == k - 1 and int((inside & (e == e[ip])).sum()) == 1
    if first > 0:
        plo, phi = C.FIRST_BLOCK[first - 1]
        assert not np.all((t >= plo) & (t < phi), axis=1).any()
    # the second block holds both; ub lies between what the shell before it and what it proves
    lo, hi = C.FIRST_BLOCK[sh2]
    inside2 = np.all((t >= lo) & (t < hi), axis=1)
    assert inside2[im] and inside2[ix] and np.all(inside2[inside])
    assert K.PROVEN[sh2 - 1] ** 2 < ub < K.PROVEN[sh2] ** 2 and ub > K.PROVEN[first] ** 2
    if "heavy" in case.name:
        assert int(inside.sum()) <= K.HEAVY < int(inside2.sum())
    # the answer by exact integer arithmetic: the k - 1 nearer points, then M -- P displaced, X out
    order = np.lexsort((np.arange(t.shape[0]), e))[:k]
    assert order[k - 1] == im and ip not in order and ix not in order
    assert np.array_equal(K.reference(case)[0], np.tile(order.astype(np.int32), (case.queries.size, 1)))


def test_fill_cases_cover_the_turn_edges_and_every_list_length():
    assert {K.compiled_lengths(kt, k) for kt, k in C.COMBOS} == {(8, 5, 0), (10, 5, 0), (16, 5, 16), (16, 8, 16), (16, 16, 16)}
    assert {kt for kt, _ in C.COMBOS} == {K.EDGE, K.PLANE}
    for kt, k in C.COMBOS:
        kmax, u = C.lane_lists(kt, k)
        assert kmax >= k
        sizes = {c.target.size for c in C.CASES if c.name.startswith("fill_") and c.name.endswith(f"_{K.TYPE_NAME[kt]}{k}") and "heavy" not in c.name}
        assert sizes >= {1, 15, 16, 17, 31, 32, 33, kmax * 8 - 1, kmax * 8 + 1}
        assert C.BY_NAME[f"fill_heavy_first_193_{K.TYPE_NAME[kt]}{k}"].target.size == 193 + 2
        assert {C.BY_NAME[f"whole_target_{m}_{K.TYPE_NAME[kt]}{k}"].target.size for m in (1, 2, 63, 64, 65, 64 * kmax + 1)} == {1, 2, 63, 64, 65, 64 * kmax + 1}
        # a covered grid: at most two cells an axis
        for c in C.CASES:
            if c.name.startswith("fill_") and "heavy" not in c.name:
                assert all(d <= 2 for d in K.grid_levels(K.xyz32(c.target), c.cell)[0][1])


def test_case_construction_is_deterministic():
    again = C.build_cases()
    assert [c.name for c in again] == [c.name for c in C.CASES]
    for a, b in zip(again, C.CASES):
        assert a.target.tobytes() == b.target.tobytes() and a.queries.tobytes() == b.queries.tobytes()
