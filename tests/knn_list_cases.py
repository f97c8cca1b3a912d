"""Cases for the list keeping of the exact kNN search (LaneList, group_min, scan_rows of lsa_match_fused.hip): keys in the
f64 denormal range, lists that fill exactly at a turn's edge, and candidates exactly at and one ulp beyond the k-th
distance the first scan hands to the second (the bound any pruning of the second scan has to respect).  Built from the helpers of tests/knn_cases.py and held to its brute_knn; needs neither a GPU nor the
oracle.  tests/test_knn_key_order.py checks what the constructions claim, tests/test_gpu_knn_list_keeping.py runs them.

Every family runs at the six (type, k) that between them select all five compiled list lengths and every LaneList size:
edges 8, 10, 16 -> <8,5,0> <10,5,0> <16,5,16>, planes 5, 8, 16 -> <8,5,0> <16,8,16> <16,16,16>."""
import numpy as np

import knn_cases as K
from knn_cases import EDGE, PLANE, SITE, Case, anchored, params, points

COMBOS = ((EDGE, 8), (EDGE, 10), (EDGE, 16), (PLANE, 5), (PLANE, 8), (PLANE, 16))
OFFSETS = (1e-20, 3e-20, 4e-20)  # squared: float32 denormals with bits below (the first two) and just above 0x00100000
F32 = np.float32


def kernel_d2(q, p):
    """float32 squared distance in the kernels' expression order, one rounding per operation"""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    dx, dy, dz = F32(q[0] - p[0]), F32(q[1] - p[1]), F32(q[2] - p[2])
    return F32(F32(F32(dx * dx) + F32(dy * dy)) + F32(dz * dz))


def lane_lists(ktype, k):
    """KMAX of the lanes' lists and the candidates a lane takes per turn (scan_rows: U = 2 for lists of 8 and more)"""
    kmax = K.compiled_lengths(ktype, k)[0 if ktype == EDGE else 1]
    return kmax, (2 if kmax >= 8 else 4)


# ------------------------------------------------------------------------------------------------ zero and denormal distances
def zero_distances(ktype, k):
    """Queries exactly ON target points.  Two `full` sites are present k + 3 times each (their copies spread over the array):
    whole lists have distance bits 0 and are ordered by index alone.  Two `thin` sites, at x = 0 exactly, are present
    twice, and next to each lie two copies each of the points offset by 1e-20, 3e-20 and 4e-20 in x: squared, 1e-40 and
    9e-40 have distance bits below 0x00100000 (f64 denormals as keys), 1.6e-39 just above.  A thin site's list is two
    zeros, then the six offset points in order of distance, ties by index, then normal distances.  Sites are 1.5 to 4
    apart in a box of 6 cells: whichever blocks the search scans, the lists must be brute force's."""
    full = [np.array([2.5, 1.0, 0.5]), np.array([4.0, 5.5, 3.0])]
    thin = [np.array([0.0, 0.0, 0.0]), np.array([0.0, 3.0, 1.5])]
    rows = []
    for c in range(k + 3):
        rows += [full[0], full[1]]
        if c < 2:
            for s in thin:
                rows += [s] + [s + np.array([o, 0.0, 0.0]) for o in OFFSETS]
    # a scattering of ordinary points so that every list is filled whatever k
    rng = np.random.default_rng(300 + k)
    rows += list(rng.uniform(0.0, 6.0, (2 * k, 3)))
    sites = full + thin
    q = np.array([sites[i % 4] for i in range(16)])
    return Case(f"zero_denormal_{K.TYPE_NAME[ktype]}{k}", points(np.array(rows)), points(q), ktype, k, params(ktype, k), 1.0, frozenset({"no_far"}))


# ------------------------------------------------------------------------------------------------ fill levels
def fill_counts(ktype, k):
    kmax, _ = lane_lists(ktype, k)
    return sorted({1, 2 * 8 - 1, 2 * 8, 2 * 8 + 1, 4 * 8 - 1, 4 * 8, 4 * 8 + 1, kmax * 8 - 1, kmax * 8 + 1})


def fill_level(ktype, k, n):
    """A block of exactly n candidates: the whole target is n points within 1.5 m (at most 2 cells per axis: any 3^3 block
    covers the grid, as knn_cases.covered), so every query scans shell 0 with n candidates dealt round robin to 8 lanes --
    lanes with fewer candidates than a turn of U takes (n = 1, U * 8 - 1), lists that fill exactly at a turn's edge
    (U * 8, U * 8 + 1) and exactly when every lane's list is full (KMAX * 8 - 1, KMAX * 8 + 1), for U = 2 and 4.  The points are in
    random order, so the nearest land on any lane and in any turn."""
    rng = np.random.default_rng(400 + 17 * n + k)
    return Case(f"fill_{n}_{K.TYPE_NAME[ktype]}{k}", points(rng.uniform(0.0, 1.5, (n, 3))), points(rng.uniform(-1.0, 2.5, (12, 3))), ktype, k,
                params(ktype, k), 1.0, frozenset({"at_once", "shell0", "no_tail", "no_far"}))


def heavy_193(ktype, k):
    """the 64-lane scan: knn_cases.heavy_first with 193 candidates (3 per lane and one lane with 4)"""
    c = K.heavy_first(ktype, k, 193)
    c.name = "fill_" + c.name
    return c


def whole_target(ktype, k, m):
    """The whole-target search over m points (search_whole_target: 64 lanes, point c to lane c mod 64), through the
    construction of knn_cases.isolated_tail: the points sit in two opposite corners of the anchored box (the anchors are the
    first two of them), the queries at S, whose largest block [16, 128) holds none of them: no block holds k points and
    none covers the grid.  m = 1 cannot be reached this way -- a single point's grid is one cell, which any block covers
    (whole_target_single: it is settled by shell 0) -- so the smallest is m = 2, the anchors alone."""
    rng = np.random.default_rng(500 + m)
    a, b = (m - 2) // 2, (m - 2) - (m - 2) // 2
    clumps = [K.clump(rng, [1.0, 1.0, 1.0], a, 0.5), K.clump(rng, [142.5, 142.5, 142.5], b, 0.5)]
    return anchored(f"whole_target_{m}_{K.TYPE_NAME[ktype]}{k}", ktype, k, clumps, K.site_queries(rng, 6), {"tail", "at_once", "no_far"})


def whole_target_single(ktype, k):
    rng = np.random.default_rng(501)
    return Case(f"whole_target_1_{K.TYPE_NAME[ktype]}{k}", points([[3.0, -2.0, 1.0]]), points(rng.uniform(-50.0, 50.0, (6, 3))), ktype, k,
                params(ktype, k), 1.0, frozenset({"at_once", "no_tail", "no_far"}))


# ------------------------------------------------------------------------------------------------ bound of the second scan
# Per second-scan route (the shells of knn_cases.second_scan): the query's x (y = z = 72.5), the first block F, the offset
# d along x of the first scan's k-th neighbour P = q + (d, 0, 0), the x offset of the k - 1 nearer points, and whether F is
# shell 0 (taken at 3k points: 2k fillers beyond P, at P's x on the quarter lattice of F).  q sits off the centre of F where F is symmetric about S, so that the
# mirror image M = q - (d, 0, 0) falls outside F and inside the second block:
#   sh2  F         q.x    P.x     M.x     ub = d^2   proven^2 of F .. of sh2 (cell = 1)
#   1    [71, 74)  72.25  73.75   70.75   2.25       0.998 .. 3.996         M in [70, 75)
#   2    [71, 74)  72.25  73.75   70.75   4.5 (P, M also +- 1.5 in y: q.y = 72.25)   3.996 < 4.5 < 15.97, M in [68, 80)
#   3    [68, 80)  72.5   78.5    66.5    36         15.97 .. 63.87         M in [64, 84), P outside [70, 75)
#   4    [64, 84)  72.5   82.5    62.5    100        63.87 .. 255.5         M in [48, 96), P outside [68, 80)
#   5    [48, 96)  72.5   48.5    96.5    576        255.5 .. 1021.9        M in [32, 112), P outside [64, 84)
#   6    [32, 112) 72.5   32.5    112.5   1600       1021.9 .. 2299.4       M in [16, 128), P outside [48, 96)
# All coordinates are halves and quarters of a cell: dx = -d and +d square to the same float, the other terms are equal.
# M comes EARLIER in the target than P (smaller index): the second scan must take it at d2 == ub and it displaces P.
# A third point X = M + (0, 0, e) has d2 exactly one ulp above ub (e a multiple of 2^-17 found by search and asserted): it
# must stay out.
BOUND_GEOMETRY = {1: (72.25, 72.5, 0, 1.5, 0.0, 0.75), 2: (72.25, 72.25, 0, 1.5, 1.5, 0.75), 3: (72.5, 72.5, 2, 6.0, 0.0, 4.0),
                  4: (72.5, 72.5, 3, 10.0, 0.0, 9.0), 5: (72.5, 72.5, 4, -24.0, 0.0, -23.0), 6: (72.5, 72.5, 5, -40.0, 0.0, -39.0)}
FIRST_BLOCK = {0: (71, 74), 1: (70, 75), 2: (68, 80), 3: (64, 84), 4: (48, 96), 5: (32, 112), 6: (16, 128)}


def one_ulp_beyond(q, m, ub):
    """a point next to m whose float32 squared distance from q is exactly the float after ub"""
    want = np.nextafter(F32(ub), F32(np.inf))
    for j in range(1, 1 << 14):
        x = np.array([m[0], m[1], m[2] + j * 2.0 ** -17])
        if kernel_d2(q, x) == want:
            return x
    raise AssertionError("no point one ulp beyond the bound")


def bound_points(sh2, k):
    qx, qy, first, d, dy, near = BOUND_GEOMETRY[sh2]
    q = np.array([qx, qy, 72.5])
    P, M = q + [d, dy, 0.0], q - [d, dy, 0.0]
    ub = kernel_d2(q, P)
    # k - 1 nearer points, on quarter offsets in y and z beside the x offset `near` (all inside F, all nearer than P)
    offs = [(a, b) for a in (0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75) for b in (0.0, 0.25, -0.25)][:k - 1]
    nearer = [q + [near, a, b] for a, b in offs]
    fillers = []
    if first == 0:
        # shell 0 is scanned first at 3k points: 2k more inside F, beyond P (same x, off in y and z)
        grid = [np.array([P[0], y, z]) for y in np.arange(71.0, 74.0, 0.25) for z in np.arange(71.0, 74.0, 0.25)]
        fillers = [g for g in grid if kernel_d2(q, g) > ub][:2 * k]
        assert len(fillers) == 2 * k
    X = one_ulp_beyond(q, M, ub)
    return q, P, M, X, nearer, fillers, ub


def bound_case(sh2, ktype, k, heavy=False):
    """target order: anchors, M, X, the nearer points, P, the fillers (, the heavy second block)"""
    q, P, M, X, nearer, fillers, ub = bound_points(sh2, k)
    first = BOUND_GEOMETRY[sh2][2]
    clumps = [np.array([M, X]), np.array(nearer + [P]).reshape(-1, 3)]
    if fillers:
        clumps.append(np.array(fillers))
    if heavy:
        # knn_cases.heavy_second: 300 more points in shell 1 outside shell 0, all beyond ub (x >= 74.25: dx >= 2)
        g = np.array([[x, y, z] for x in (74.25, 74.5, 74.75) for y in np.arange(70.0, 75.0, 0.5) for z in np.arange(70.0, 75.0, 0.5)])[:300]
        clumps.append(g)
    routes = {"second", "no_tail", "no_far", "light"} | ({"shell0", "within2"} if first == 0 else {"not_shell0"}) | ({"beyond2"} if first >= 3 else {"within2"})
    name = f"bound_{'heavy' if heavy else 'sh%d' % sh2}_{K.TYPE_NAME[ktype]}{k}"
    c = anchored(name, ktype, k, clumps, np.tile(q, (3, 1)), routes)
    c.tags = {"bound": (sh2, first, float(ub)), "mirror": 2, "beyond": 3, "kth": 2 + 2 + k - 1}
    return c


def build_cases():
    cs = []
    for kt, k in COMBOS:
        kmax, _ = lane_lists(kt, k)
        cs.append(zero_distances(kt, k))
        cs += [fill_level(kt, k, n) for n in fill_counts(kt, k)]
        cs.append(heavy_193(kt, k))
        cs.append(whole_target_single(kt, k))
        cs += [whole_target(kt, k, m) for m in (2, 63, 64, 65, 64 * kmax + 1)]
        cs += [bound_case(sh2, kt, k) for sh2 in (1, 2, 3, 4, 5, 6)]
        cs.append(bound_case(1, kt, k, heavy=True))
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    for c in cs:
        assert c.routes <= K.ROUTE_TAGS and c.target.size <= 4096 and c.queries.size <= 64
    return cs


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
