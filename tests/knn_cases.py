"""Cases that force every route of the exact kNN search (lsa_match_fused.hip, lsa_match_staged.hip) and every shape of
the grid build (lsa_target.hip), and the reference they are held to.  Needs neither a GPU nor the oracle.

Reference: brute force over all target points in float32, in the kernels' own expression order
(dx * dx + dy * dy) + dz * dz with d = query - point, one rounding per operation (numpy float32 arrays round every
operation once), ordered by (distance bits, target index).  It shares nothing with the search but that expression.

Grid geometry the constructions rely on (lsa_target.hip, DESIGN.md "search"): the origin is the minimum corner of the
target's bounding box; level 0 has cells of `cell`, level 1 of 4 x, level 2 of 16 x -- unless a level exceeds its budget
(4 194 304, 65 600 and 1 088 cells), then its cell and every coarser one grows by 1.26 until it fits; dims = floor(extent /
cell) + 1 per axis.  A query's shells are the blocks of 3^3, 5^3 cells of level 0 (shells 0, 1), 3^3, 5^3 of level 1
(shells 2, 3) and 3^3, 5^3, 7^3 of level 2 (shells 4, 5, 6) around the cell it falls in; a block of radius r cells proves
everything closer than (r - 0.001) cells (+ the squared distance of the query to the box, times 0.999).  At cell = 1 the
proven radii are 0.999, 1.999, 3.996, 7.992, 15.984, 31.968, 47.952.

The routed cases live in one "anchored" box: two target points at (0, 0, 0) and (143.5, 143.5, 143.5) fix the grid to 144 /
36 / 9 cells per axis at cells of exactly 1, 4 and 16 (all three within budget: 2 985 984, 46 656 and 729 cells), and the
query site S = (72.5, 72.5, 72.5) falls in level-0 cell 72, level-1 cell 18 = [72, 76) and level-2 cell 4 = [64, 80) on
every axis.  Its blocks are therefore, per axis,
    shell 0 [71, 74)   shell 1 [70, 75)   shell 2 [68, 80)   shell 3 [64, 84)   shell 4 [48, 96)   shell 5 [32, 112)
    shell 6 [16, 128)
and the anchors (more than 120 away) are in none of them.  The queries of a site are S + U(-0.05, 0.05): they stay in S's
cells.  Each builder's comment derives its route from these numbers; tests/test_gpu_knn_routes.py confirms it with the
counters of LSA_ROUTE_STATS."""
from dataclasses import dataclass, field

import numpy as np

from lidarslam_amd import KNN_MAX  # noqa: F401  (slots per query of the lists the hook hands out)
from lidarslam_amd._native import BLOB, EDGE, PLANE, POINT_DTYPE, MatchParams

BOX = 143.5
SITE = np.array([72.5, 72.5, 72.5])
NEAR = np.array([8.5, 8.5, 8.5])  # a second site, 111 away from SITE and outside its largest block [16, 128): its own shell 0 is [7, 10)
PROVEN = [0.999, 1.999, 3.996, 7.992, 15.984, 31.968, 47.952]  # radius a shell proves at cell = 1
HEAVY = 192  # kHeavyCandidates: a block with more candidates is scanned by the whole wavefront
LEVEL_BUDGET = [1 << 22, (1 << 16) + 64, (1 << 10) + 64]

# route tags -> what tests/test_gpu_knn_routes.py asserts of the counters (route = lsa_match_route_stats()[2:8])
#   second     every query scanned a second block:              route[0] == nq, none handed to the whole-target search
#   at_once    no query scanned a second block:                 route[0] == 0
#   shell0     every first block was shell 0:                   route[4] == nq
#   not_shell0 no first block was shell 0:                      route[4] == 0
#   beyond2    every first block was beyond shell 2:            route[1] == nq
#   within2    no first block was beyond shell 2:               route[1] == 0
#   far_counts NEIGHBORS_TOO_FAR by the counts alone:           route[3] == number of -1 entries > 0
#   far_scan   ... after the first scan (no counter sees it):   route[3] == 0 while -1 entries > 0
#   no_far     no exit by the counts:                           route[3] == 0
#   tail       every query went to the whole-target search:     slow == nq
#   no_tail    none did:                                        slow == 0
#   all_heavy  only whole-wavefront scans:                      route[2] > 0, longest lane walk route[5] == 0
#   light      lane walks happened:                             route[5] > 0
ROUTE_TAGS = {"second", "at_once", "shell0", "not_shell0", "beyond2", "within2", "far_counts", "far_scan", "no_far", "tail", "no_tail", "all_heavy", "light"}


@dataclass
class Case:
    name: str
    target: np.ndarray            # POINT_DTYPE
    queries: np.ndarray           # POINT_DTYPE, BASE coordinates (world coordinates when pose is None)
    ktype: int
    k: int
    mp: MatchParams
    cell: float = 1.0
    routes: frozenset = frozenset()
    pose: np.ndarray = None       # None: identity
    sweep: bool = False           # run every lane count and round count of the staged form
    anchored: bool = False        # lives in the anchored box: cells of exactly 1, 4, 16
    lattice: bool = False         # every coordinate a multiple of 0.5: float32 distances are exact
    far_share: tuple = (0.0, 0.0)  # bounds (exclusive unless equal) of the share of queries whose k-th neighbour is beyond max_neighbors_distance
    settled_within: float = None  # every query's k-th squared distance is below this (the radius its first block proves)
    tags: dict = field(default_factory=dict)

    @property
    def max_dist2(self):
        return float(self.mp.max_neighbors_distance) ** 2


def points(xyz, laser_id=None):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3).astype(np.float32)
    p = np.zeros(xyz.shape[0], POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    # rings for the edge filters: neighbouring indices on different rings, as keypoints of a scan are
    p["laser_id"] = (np.arange(xyz.shape[0]) % 16) if laser_id is None else laser_id
    p["time"] = -0.05
    return p


def xyz32(p):
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


def params(ktype, k, max_dist=1000.0, single=0):
    """the searched type asks for k; a far rejection distance unless the case is about it"""
    return MatchParams(single_edge_per_ring=single, edge_nb_neighbors=k if ktype == EDGE else 10, edge_min_nb_neighbors=2,
                       plane_nb_neighbors=k if ktype == PLANE else 5, blob_nb_neighbors=k if ktype == BLOB else 10,
                       max_neighbors_distance=max_dist, edge_max_model_error=0.2, plane_max_model_error=0.2, saturation_distance=2.0)


def compiled_lengths(ktype, k):
    """the instantiation <KE, KP, KB> of the fused kernels a single-type match selects (enqueue_fused_match: the other
    types count as k = 1, blobs are present only when they are the type matched)"""
    ke, kp, blobs = (k if ktype == EDGE else 1), (k if ktype == PLANE else 1), ktype == BLOB
    if not blobs and ke <= 8 and kp <= 5:
        return (8, 5, 0)
    if not blobs and ke <= 10 and kp <= 5:
        return (10, 5, 0)
    if kp <= 5:
        return (16, 5, 16)
    return (16, 8, 16) if kp <= 8 else (16, 16, 16)


# ------------------------------------------------------------------------------------------------ reference
def brute_knn(target_xyz, query_xyz, k, chunk=128):
    """(idx (n, min(k, m)) int32, d2 (n, min(k, m)) float32): the k nearest target points of every query, ascending by
    (float32 squared distance, index)"""
    t = np.ascontiguousarray(target_xyz, np.float32)
    q = np.ascontiguousarray(query_xyz, np.float32)
    m, kk = t.shape[0], min(k, t.shape[0])
    idx = np.zeros((q.shape[0], kk), np.int32)
    d2 = np.zeros((q.shape[0], kk), np.float32)
    ids = np.arange(m, dtype=np.uint64)
    for a in range(0, q.shape[0], chunk):
        qq = q[a:a + chunk]
        dx = qq[:, None, 0] - t[None, :, 0]
        dy = qq[:, None, 1] - t[None, :, 1]
        dz = qq[:, None, 2] - t[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]  # distances are >= 0: bit order is value order
        best = np.sort(np.partition(key, kk - 1, axis=1)[:, :kk], axis=1) if kk > 0 else key[:, :0]
        idx[a:a + chunk] = (best & np.uint64(0xFFFFFFFF)).astype(np.int32)
        d2[a:a + chunk] = (best >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx, d2


def brute_knn_f64(target_xyz, query_xyz, k):
    """the same in float64 (idx, d2 float64), for the trust checks of the float32 reference"""
    t = np.asarray(target_xyz, np.float64)
    q = np.asarray(query_xyz, np.float64)
    kk = min(k + 1, t.shape[0])  # one more: the gap behind the k-th place
    d = ((q[:, None, :] - t[None, :, :]) ** 2).sum(2)
    order = np.lexsort((np.broadcast_to(np.arange(t.shape[0]), d.shape), d), axis=1)[:, :kk]
    return order.astype(np.int32), np.take_along_axis(d, order, 1)


def brute_knn_int(target_xyz, query_xyz, k):
    """lattice cases (every coordinate a multiple of 0.5): exact integer arithmetic on the doubled coordinates"""
    t = np.rint(np.asarray(target_xyz, np.float64) * 2).astype(np.int64)
    q = np.rint(np.asarray(query_xyz, np.float64) * 2).astype(np.int64)
    assert np.array_equal(t, np.asarray(target_xyz, np.float64) * 2) and np.array_equal(q, np.asarray(query_xyz, np.float64) * 2)
    kk = min(k, t.shape[0])
    d = ((q[:, None, :] - t[None, :, :]) ** 2).sum(2)  # 4 x the squared distance
    order = np.lexsort((np.broadcast_to(np.arange(t.shape[0]), d.shape), d), axis=1)[:, :kk]
    return order.astype(np.int32), np.take_along_axis(d, order, 1)


def grid_levels(target_xyz, cell_hint):
    """[(cell, dims)] of the three levels as k_grid_setup derives them (float32): used to check what the cases CLAIM of
    the geometry (neat cells, which levels grow), never to predict a result"""
    t = np.asarray(target_xyz, np.float32)
    mn, mx = t.min(0), t.max(0)
    cell, out = np.float32(cell_hint), []
    for level in range(3):
        if level > 0:
            cell = np.float32(cell * np.float32(4.0))
        while True:
            dims = [int(np.floor(np.float32(np.float32(mx[d] - mn[d]) / cell))) + 1 for d in range(3)]
            if float(dims[0]) * dims[1] * dims[2] <= LEVEL_BUDGET[level]:
                break
            cell = np.float32(cell * np.float32(1.26))
        out.append((float(cell), dims))
    return out


# ------------------------------------------------------------------------------------------------ building blocks
ANCHORS = np.array([[0.0, 0.0, 0.0], [BOX, BOX, BOX]])


def clump(rng, centre, n, spread):
    return np.asarray(centre)[None, :] + rng.uniform(-spread, spread, (n, 3))


def site_queries(rng, n, centre=SITE):
    return np.asarray(centre)[None, :] + rng.uniform(-0.05, 0.05, (n, 3))


def anchored(name, ktype, k, clumps, queries, routes, **kw):
    mp = kw.pop("mp", None) or params(ktype, k)
    return Case(name, points(np.concatenate([ANCHORS] + list(clumps))), points(queries), ktype, k, mp, 1.0, frozenset(routes), anchored=True, **kw)


TYPE_NAME = {EDGE: "edge", PLANE: "plane", BLOB: "blob"}


def second_scan(sh2, ktype, k, seed=1):
    """Second scan into shell sh2.  A cluster sits at S + (o, o, o) +- 0.05, in a corner cell of the first block F and
    outside the next smaller one, so F is the block scanned first (shell 0 is taken at kFill x k = 3k points, otherwise
    shell 2, which holds the same points, would be: the cluster has exactly 3k there; where F is shell 2 or later it is the
    first block to hold k points and the cluster has exactly k).  Its distance d = sqrt(3) (o -+ 0.1)
    lies beyond the radius F proves and inside the radius shell sh2 proves, so the k-th best seen after the first scan
    bounds the k-th distance between the two and the first shell that proves more is sh2:
        sh2  F  o      d^2 in            proven^2 of F, of sh2 - 1, of sh2
        1    0  0.8    [1.47, 2.43]      0.998, -, 3.996      (in [71, 74): 73.3)
        2    0  1.4    [5.07, 6.75]      0.998, 3.996, 15.97  (in [71, 74): 73.9)
        3    2  3.8    [41.1, 45.6]      15.97, -, 63.87      (in [76, 80), outside [70, 75))
        4    3  7.8    [177.9, 187.2]    63.87, -, 255.5      (in [80, 84), outside [68, 80))
        5    4  18     [961.2, 982.8]    255.5, -, 1021.9     (in [48, 96), outside [64, 84))
        6    5  24.5   [1786, 1816]      1021.9, -, 2299.4    (in [32, 112), outside [48, 96))
    Shells 1 and 2 are still in their tables from the first round trip (kept), 3 .. 6 are fetched.  For sh2 >= 2 a few
    decoys (k // 2 points) sit at S - (e, 0, 0), outside F but inside shell sh2 and NEARER than the cluster (e = 1.7, 5, 9,
    25, 41): the first scan cannot see them, the second must, and they head the answer."""
    o, e = {1: (0.8, None), 2: (1.4, 1.7), 3: (3.8, 5.0), 4: (7.8, 9.0), 5: (18.0, 25.0), 6: (24.5, 41.0)}[sh2]
    rng = np.random.default_rng(100 * sh2 + seed)
    first = {1: 0, 2: 0, 3: 2, 4: 3, 5: 4, 6: 5}[sh2]
    clumps = [clump(rng, SITE + o, 3 * k if first == 0 else k, 0.05)]
    if e is not None:
        clumps.append(clump(rng, SITE - np.array([e, 0.0, 0.0]), k // 2, 0.02))
    routes = {"second", "no_tail", "no_far", "light"} | ({"shell0", "within2"} if first == 0 else {"not_shell0"}) | ({"beyond2"} if first >= 3 else {"within2"})
    return anchored(f"second_scan_sh{sh2}_{TYPE_NAME[ktype]}{k}", ktype, k, clumps, site_queries(rng, 40), routes, sweep=True)


def guard_band(ktype, k):
    """What a block proves is r cells and not a hair more: the queries sit at x = 72.99, next to the face x = 73 of their
    cell, 3k points at x = 71.945 (distance 1.045 +- 0.006, inside shell 0 [71, 74)) and k // 2 + 1 decoys at x = 74.02, just
    OUTSIDE shell 0, at distance 1.03 +- 0.006 -- nearer than the cluster.  Shell 0 proves 0.999 < 1.039, so the second scan
    (shell 1, ub <= 1.051^2 < 3.996) has to happen and the decoys head the answer; a proof that claimed 1.05 cells would
    settle the query on the cluster alone."""
    rng = np.random.default_rng(6)
    q = np.array([72.99, 72.5, 72.5]) + rng.uniform(-0.004, 0.004, (40, 3))
    clumps = [clump(rng, [71.945, 72.5, 72.5], 3 * k, 0.002), clump(rng, [74.02, 72.5, 72.5], k // 2 + 1, 0.002)]
    return anchored(f"guard_band_{TYPE_NAME[ktype]}{k}", ktype, k, clumps, q, {"second", "shell0", "within2", "no_tail", "no_far", "light"}, sweep=True)


def unproven_tail(ktype, k):
    """First scan whose k-th distance no shell proves: the cluster (k points) sits at S + 37.5 = 110, inside shell 5
    [32, 112) and outside shell 4 [48, 96), so shell 5 is the first block holding k points; d^2 = 3 x 37.5^2 = 4219 is
    beyond what even shell 6 proves (2299.4): whole-target search, no second scan."""
    rng = np.random.default_rng(7)
    return anchored(f"tail_unproven_{TYPE_NAME[ktype]}{k}", ktype, k, [clump(rng, SITE + 37.5, k, 0.05)], site_queries(rng, 40),
                    {"tail", "at_once", "beyond2", "not_shell0", "no_far"})


def isolated_tail(k=8):
    """No block holds k points: 6 points in each of two opposite corners of the box (m = 14 with the anchors >= k = 8);
    shell 6 of S is [16, 128) and holds none of them, and the queries 40 cells outside the face x = 0 (clamped to cell 0:
    shell 6 is [0, 64) in x and [16, 128) in y, z) see none either.  Edges have no rejection distance: whole-target search."""
    rng = np.random.default_rng(8)
    q = np.concatenate([site_queries(rng, 20), site_queries(rng, 20, [-40.0, 72.5, 72.5])])
    return anchored(f"tail_isolated_edge{k}", EDGE, k, [clump(rng, [1.0, 1.0, 1.0], 6, 0.5), clump(rng, [142.5, 142.5, 142.5], 6, 0.5)], q,
                    {"tail", "at_once", "no_far"})


def settled_beyond2(ktype, k):
    """First block beyond shell 2, settled at once: 2k points at S - (5.5, 0, 0) +- 0.05, i.e. x = 67: outside shell 2
    [68, 80), inside shell 3 [64, 84), at distance 5.5 +- 0.15 < 7.992.  Shells 0 .. 2 hold nothing."""
    rng = np.random.default_rng(9)
    return anchored(f"settled_beyond2_{TYPE_NAME[ktype]}{k}", ktype, k, [clump(rng, SITE - np.array([5.5, 0.0, 0.0]), 2 * k, 0.05)], site_queries(rng, 40),
                    {"at_once", "beyond2", "not_shell0", "no_tail", "no_far", "light"}, settled_within=7.992 ** 2)


def far_case(which, ktype, k, max_dist):
    """The three NEIGHBORS_TOO_FAR exits (planes and blobs; m >= k).  Half of the queries sit at NEAR inside a clump of 3k
    points (+- 0.25: all within 0.52 < 0.9, settled in shell 0 whatever the rejection distance), half at S:
      counts3  max_dist 0.9 (far_d2 0.81 < 0.998 = shell 0's proof): nothing within 110 of S, shell 0 holds 0 < k points and
               proves more than the rejection distance -- the exit by the counts of the first three shells, and the only
               one reachable: a query either has 3k points in shell 0 or none.
      later    max_dist 5 / 10 / 20 / 40 (far_d2 25, 100, 400, 1600): shells 0 .. 2 prove at most 15.97 < far_d2, so their
               counts cannot reject; shell 3 / 4 / 5 / 6 is the first to prove more (63.87, 255.5, 1021.9, 2299.4) and holds
               nothing -- the exit by the counts of a later shell.
      scan     max_dist 0.9: 3k points at S + 0.8 (the sh2 = 1 construction): shell 0 holds them, is scanned, none lies
               inside 0.999 while 0.998 > far_d2 -- the exit after the first scan.  No counter sees this one."""
    rng = np.random.default_rng({"counts3": 11, "later": 12, "scan": 13}[which] + int(max_dist))
    clumps = [clump(rng, NEAR, 3 * k, 0.25)]
    if which == "scan":
        clumps.append(clump(rng, SITE + 0.8, 3 * k, 0.05))
    q = np.empty((40, 3))
    q[0::2], q[1::2] = site_queries(rng, 20, NEAR), site_queries(rng, 20)
    routes = {"no_tail", "at_once"} | ({"far_scan", "shell0"} if which == "scan" else {"far_counts"})
    return anchored(f"far_{which}_{TYPE_NAME[ktype]}{k}_d{max_dist:g}", ktype, k, clumps, q, routes, mp=params(ktype, k, max_dist), far_share=(0.0, 1.0))


def heavy_first(ktype, k, n):
    """n points within +- 0.25 of S: shell 0 holds n >= 3k candidates and the k-th is within 0.52 < 0.999.  n > 192: every
    first scan is a whole-wavefront scan and no lane walks (route[5] == 0); n == 192 stays with the lanes."""
    rng = np.random.default_rng(20 + n)
    routes = {"at_once", "shell0", "no_tail", "no_far"} | ({"all_heavy"} if n > HEAVY else {"light"})
    return anchored(f"heavy_first_{n}_{TYPE_NAME[ktype]}{k}", ktype, k, [clump(rng, SITE, n, 0.25)], site_queries(rng, 40), routes, settled_within=0.999 ** 2)


def heavy_second(ktype, k):
    """The sh2 = 1 construction (3k points at S + 0.8) plus 300 points at S + 1.9 +- 0.05 = 74.4: outside shell 0 [71, 74),
    inside shell 1 [70, 75).  First scan light (3k candidates), second scan heavy (3k + 300 > 192); the answer is still the
    cluster's (d^2 <= 2.43 against >= 3 x 1.8^2 = 9.7)."""
    rng = np.random.default_rng(31)
    return anchored(f"heavy_second_{TYPE_NAME[ktype]}{k}", ktype, k, [clump(rng, SITE + 0.8, 3 * k, 0.05), clump(rng, SITE + 1.9, 300, 0.05)], site_queries(rng, 40),
                    {"second", "shell0", "within2", "no_tail", "no_far", "light"}, sweep=True)


def heavy_alternating(ktype, k):
    """Adjacent queries alternate between a clump of 300 points at S (heavy first scan) and a clump of 3k points at NEAR
    (light): in every wavefront heavy and light groups sit side by side -- merge_lists(.., take = false) for the heavy
    groups while the light ones merge, and the LDS slots.  Deliberately mixed: both counters are only > 0."""
    rng = np.random.default_rng(32)
    q = np.empty((66, 3))
    q[0::2], q[1::2] = site_queries(rng, 33), site_queries(rng, 33, NEAR)
    return anchored(f"heavy_alternating_{TYPE_NAME[ktype]}{k}", ktype, k, [clump(rng, SITE, 300, 0.25), clump(rng, NEAR, 3 * k, 0.25)], q,
                    {"at_once", "shell0", "no_tail", "no_far", "light"}, settled_within=0.999 ** 2, tags={"heavy_too": True})


def jittered_lattice(rng, lo, n, spacing, jitter):
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3) * spacing
    return np.asarray(lo)[None, :] + g + rng.uniform(-jitter, jitter, g.shape)


def dense(ktype, k, nq=64, name=None, single=0):
    """Settled in the first scan with shell 0 first: a jittered lattice (spacing 0.5 +- 0.1, 17^3 points over 8 m, 8 per unit
    cell) and queries at least 2 cells inside it: shell 0 holds about 6^3 = 216 >= 3k points, and a ball of 0.999 holds 33 on
    average, k of them for certain (checked against the reference by tests/test_knn_reference.py)."""
    rng = np.random.default_rng(40)
    t = jittered_lattice(rng, [0.0, 0.0, 0.0], 17, 0.5, 0.1)
    q = rng.uniform(2.5, 5.5, (nq, 3))
    return Case(name or f"dense_{TYPE_NAME[ktype]}{k}{'_ring' if single else ''}", points(t), points(q), ktype, k, params(ktype, k, single=single), 1.0,
                frozenset({"at_once", "shell0", "within2", "no_tail", "no_far"}), settled_within=0.999 ** 2)


def ragged(nq):
    """Query counts around the 32 queries of a workgroup (G = 8 lanes each): the last groups of the last wavefront inactive"""
    return dense(PLANE, 5, nq, name=f"ragged_{nq}")


def covered(m, k=5):
    """The whole grid inside the first 3^3 block: m points within 1.5 m, so every axis has at most 2 cells and any query's
    shell 0 covers the grid (`covered`): settled by one scan whatever the distances; m < k gives NOT_ENOUGH_NEIGHBORS with
    m neighbours found.  Queries inside the box and up to 3 m around it."""
    rng = np.random.default_rng(50 + m)
    return Case(f"covered_m{m}_plane{k}", points(rng.uniform(0.0, 1.5, (m, 3))), points(rng.uniform(-3.0, 4.5, (33, 3))), PLANE, k, params(PLANE, k), 1.0,
                frozenset({"at_once", "shell0", "no_tail", "no_far"}))


def degenerate(which, ktype=PLANE, k=5):
    """Degenerate extents: all target points identical (1 x 1 x 1 cells); collinear along one axis (1 cell on the two
    others); coplanar at constant z (1 cell in z)."""
    rng = np.random.default_rng(60)
    if which == "identical":
        t = np.tile([[3.25, -1.5, 0.75]], (50, 1))
        q = t[0] + rng.uniform(-2.0, 2.0, (33, 3))
    elif which in ("line_x", "line_y", "line_z"):
        a = "xyz".index(which[-1])
        t = np.zeros((300, 3)) + [1.0, 2.0, 3.0]
        t[:, a] = np.linspace(-15.0, 15.0, 300)
        q = np.zeros((48, 3)) + [1.0, 2.0, 3.0] + rng.uniform(-1.5, 1.5, (48, 3))
        q[:, a] = rng.uniform(-18.0, 18.0, 48)
    else:
        g = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing="ij"), -1).reshape(-1, 2) * 0.5 + rng.uniform(-0.1, 0.1, (1600, 2))
        t = np.concatenate([g, np.full((1600, 1), 1.25)], 1)
        q = np.concatenate([rng.uniform(-2.0, 22.0, (48, 2)), rng.uniform(-1.0, 3.0, (48, 1))], 1)
    return Case(f"degenerate_{which}_{TYPE_NAME[ktype]}{k}", points(t), points(q), ktype, k, params(ktype, k), 1.0, frozenset({"no_far"}))


def outside_box(ktype, k):
    """Queries clamped from outside the box: a jittered lattice over [0, 9.6]^3 (spacing 0.6), queries beyond each of the six
    faces, two edges and two corners at 0.5 and at 40 cells, and exactly on the box minimum and maximum (taken from the
    float32 points themselves).  Routes are mixed on purpose (the far ones need a second scan: the box distance enters the
    proven radius)."""
    rng = np.random.default_rng(70)
    t = points(jittered_lattice(rng, [0.0, 0.0, 0.0], 17, 0.6, 0.1))
    x = xyz32(t).astype(np.float64)
    mn, mx, mid = x.min(0), x.max(0), 0.5 * (x.min(0) + x.max(0))
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (0, -1, -1), (1, 1, 1), (-1, -1, -1)]
    q = []
    for d in dirs:
        d = np.array(d, float)
        for dist in (0.5, 40.0):
            for _ in range(3):
                p = np.where(d > 0, mx + dist, np.where(d < 0, mn - dist, mid + rng.uniform(-3.0, 3.0, 3)))
                q.append(p)
    q += [mn, mx, [mn[0], mx[1], mid[2]]]
    return Case(f"outside_box_{TYPE_NAME[ktype]}{k}", t, points(q), ktype, k, params(ktype, k), 1.0, frozenset({"no_far"}))


def budget_growth(which, ktype=PLANE, k=5):
    """Budget growth (k_grid_setup's x 1.26 loop); queries in dense spots, in sparse spots and outside the box.
      level0   hint 0.02 on a 60 m cloud: 3001^3 cells -> level 0 grows 13 times (0.404), levels 1 and 2 then fit.
      flat     200 m x 200 m x 4 m at hint 0.3: level 0 grows once (0.378: 530 x 530 x 11), level 1 fits at 1.512 (133 x 133 x 3),
               level 2 (6.05: 34 x 34 x 1 = 1156 > 1088) grows once more -- its cell is 20.2 x, not 16 x level 0's.
      flat2    200 m x 200 m x 1.1 m at hint 0.25: level 0 fits (801 x 801 x 5), level 1 (1.0: 201 x 201 x 2 = 80 802 > 65 600)
               grows once, level 2 (5.04: 40 x 40 = 1600) once more: three different factors."""
    rng = np.random.default_rng(80)
    ext, hint = {"level0": ([60.0, 60.0, 60.0], 0.02), "flat": ([200.0, 200.0, 4.0], 0.3), "flat2": ([200.0, 200.0, 1.1], 0.25)}[which]
    ext = np.array(ext)
    centres = rng.uniform(0.1, 0.9, (12, 3)) * ext
    t = np.concatenate([np.zeros((1, 3)), ext[None, :], rng.uniform(0.0, 1.0, (3000, 3)) * ext] +
                       [c + rng.normal(0.0, 0.3, (400, 3)) * [1.0, 1.0, 0.2 if which != "level0" else 1.0] for c in centres])
    t = np.clip(t, 0.0, ext)
    q = np.concatenate([centres[rng.integers(0, 12, 40)] + rng.normal(0.0, 0.4, (40, 3)), rng.uniform(0.0, 1.0, (40, 3)) * ext,
                        rng.uniform(-0.3, 1.3, (24, 3)) * ext, rng.uniform(0.8, 1.0, (24, 3)) * ext])  # (the last: the far end of every level's grid)
    return Case(f"budget_{which}_{TYPE_NAME[ktype]}{k}", points(t), points(q), ktype, k, params(ktype, k), hint, frozenset({"no_far"}), tags={"grows": which})


def far_from_origin(ktype, k):
    """Negative coordinates, a box far from the origin: a jittered lattice centred at (-1000, 2000, -50), where float32 spacing
    is 6e-5 to 1.2e-4, so distances round visibly -- in the reference exactly as in the kernels."""
    rng = np.random.default_rng(90)
    c = np.array([-1000.0, 2000.0, -50.0])
    t = jittered_lattice(rng, c - 3.9, 14, 0.6, 0.1)
    q = np.concatenate([c + rng.uniform(-3.0, 3.0, (48, 3)), c + rng.uniform(-8.0, 8.0, (16, 3))])
    return Case(f"offset_box_{TYPE_NAME[ktype]}{k}", points(t), points(q), ktype, k, params(ktype, k), 1.0, frozenset({"no_far"}))


def lattice(ktype, k, duplicated=False, single=0):
    """Ties: the integer lattice {0 .. 11}^3 (one point per unit cell), queries ON lattice points, at cell centres (+ 0.5 on
    every axis: 8 nearest at equal distance, then 24, ...) and at face centres (+ 0.5 on one axis), interior and on the
    boundary.  Every distance is an exact multiple of 0.25, dozens are equal, and the k-th place falls inside a tie group
    whose members lie in different rows, lanes and -- for the shells of level 1 -- levels: only the index decides.
    duplicated: every point once more at index i + m / 2, so the two members of a tie are far apart in the cell-sorted arrays."""
    g = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    rng = np.random.default_rng(95)
    g = g[rng.permutation(g.shape[0])]  # indices unrelated to the position
    t = np.concatenate([g, g]) if duplicated else g
    base = np.concatenate([rng.integers(2, 10, (16, 3)), rng.integers(0, 12, (8, 3))]).astype(np.float64)
    q = np.concatenate([base, base + 0.5, base + [0.5, 0, 0], base + [0, 0.5, 0], base + [0, 0, 0.5]])
    return Case(f"lattice{'_dup' if duplicated else ''}_{TYPE_NAME[ktype]}{k}{'_ring' if single else ''}", points(t), points(q), ktype, k, params(ktype, k, single=single), 1.0,
                frozenset({"no_far", "no_tail"}), sweep=True, lattice=True)


def posed(ktype=EDGE, k=10):
    """One case under a real pose: the dense lattice seen from a BASE frame; the world points the search must use are
    Oracle.transform's (held to the device by test_rigid_transforms_bit_exact), the same ones the reference takes."""
    c = dense(ktype, k)
    a = 0.3
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]
    T[:3, 3] = [1.5, -2.0, 0.25]
    inv = np.linalg.inv(T)
    qb = xyz32(c.queries).astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]
    return Case(f"posed_{TYPE_NAME[ktype]}{k}", c.target, points(qb), ktype, k, c.mp, 1.0, frozenset({"no_far", "no_tail"}), pose=T)


def build_cases():
    cs = []
    # second scans into every later shell; list lengths: <10,5,0> (edge 10), <8,5,0> (plane 5, edge 8), <16,8,16> (plane 8),
    # <16,16,16> (plane 16), <16,5,16> (edge 16, blobs)
    for sh2, (kt, k) in zip((1, 2, 3, 4, 5, 6), ((EDGE, 10), (PLANE, 5), (EDGE, 16), (PLANE, 8), (BLOB, 10), (PLANE, 16))):
        cs.append(second_scan(sh2, kt, k))
    cs += [second_scan(1, PLANE, 16, seed=2), second_scan(2, EDGE, 8, seed=2), second_scan(3, PLANE, 3, seed=2), second_scan(4, EDGE, 2, seed=2)]
    cs += [guard_band(PLANE, 5), guard_band(EDGE, 10)]
    cs += [unproven_tail(EDGE, 8), unproven_tail(PLANE, 5), isolated_tail(8)]
    cs += [settled_beyond2(PLANE, 5), settled_beyond2(EDGE, 16)]
    cs += [far_case("counts3", PLANE, 5, 0.9), far_case("counts3", BLOB, 4, 0.9)]
    cs += [far_case("later", PLANE, 5, d) for d in (5.0, 10.0, 20.0, 40.0)] + [far_case("later", BLOB, 16, 5.0)]
    cs += [far_case("scan", PLANE, 8, 0.9), far_case("scan", BLOB, 10, 0.9)]
    cs += [heavy_first(PLANE, 5, 300), heavy_first(EDGE, 16, 300), heavy_first(PLANE, 5, HEAVY), heavy_first(PLANE, 5, HEAVY + 1)]
    cs += [heavy_second(EDGE, 10), heavy_second(PLANE, 16), heavy_alternating(EDGE, 8), heavy_alternating(PLANE, 16)]
    cs += [dense(PLANE, 5), dense(EDGE, 8, single=1), dense(EDGE, 10), dense(PLANE, 3), dense(EDGE, 2), dense(BLOB, 4), dense(PLANE, 16), dense(EDGE, 16)]
    cs += [ragged(n) for n in (1, 31, 32, 33)]
    cs += [covered(m) for m in (1, 4, 5, 6)]
    cs += [degenerate(w) for w in ("identical", "line_x", "line_y", "line_z", "plane_z")] + [degenerate("line_x", EDGE, 8)]
    cs += [outside_box(EDGE, 8), outside_box(PLANE, 5)]
    cs += [budget_growth("level0"), budget_growth("flat"), budget_growth("flat2", EDGE, 10)]
    cs += [far_from_origin(PLANE, 5), far_from_origin(EDGE, 10)]
    cs += [lattice(EDGE, 8, single=1), lattice(EDGE, 10), lattice(EDGE, 16), lattice(PLANE, 5), lattice(PLANE, 8), lattice(PLANE, 16), lattice(BLOB, 16)]
    cs += [lattice(PLANE, 5, duplicated=True), lattice(EDGE, 10, duplicated=True)]
    cs.append(posed())
    names = [c.name for c in cs]
    assert len(set(names)) == len(names)
    for c in cs:
        assert c.routes <= ROUTE_TAGS and c.target.size <= 16384 and c.queries.size <= 2048
    return cs


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}


def world_queries(case, O=None):
    """float32 (n, 3): the points the search uses -- the queries themselves under the identity, Oracle.transform's otherwise"""
    if case.pose is None:
        return xyz32(case.queries)
    return xyz32(O.transform(case.queries, case.pose))


_REF = {}


def reference(case, O=None):
    """brute-force lists of a case, computed once and shared (callers must not write into them)"""
    if case.name not in _REF:
        idx, d2 = brute_knn(xyz32(case.target), world_queries(case, O), case.k)
        idx.setflags(write=False)
        d2.setflags(write=False)
        _REF[case.name] = (idx, d2)
    return _REF[case.name]


def staged_handovers(case, rounds, O=None):
    """How many queries of an anchored case the staged form's first kernel hands to its second one (what
    lsa_match_slow_queries reports after a staged match).  The first kernel tries the blocks of 3^3 .. (2 rounds + 1)^3 cells
    of level 0; the last one holds every point closer than rounds - 0.001 cells (+ the distance to the box), so it settles a
    query exactly when the k-th distance -- the reference's -- lies inside that radius.  Only asked where no rejection
    distance can end a search earlier."""
    assert case.anchored and not case.name.startswith("far_") and case.target.size >= case.k
    q = world_queries(case, O).astype(np.float64)
    out = np.maximum(0.0 - q, 0.0) + np.maximum(q - (np.floor(BOX) + 1.0), 0.0)  # the grid ends at dims x cell = 144
    br = np.float32(np.float32(rounds) - np.float32(0.001))
    bound2 = (out ** 2).sum(1) * 0.999 + float(br * br)
    return int((reference(case, O)[1][:, case.k - 1].astype(np.float64) >= bound2).sum())


def beyond_rejection(case, O=None):
    """bool (n,): the reference's k-th squared distance, as double, exceeds max_neighbors_distance^2 (only asked where m >= k)"""
    idx, d2 = reference(case, O)
    if d2.shape[1] < case.k:
        return np.zeros(d2.shape[0], bool)
    return d2[:, case.k - 1].astype(np.float64) > case.max_dist2
