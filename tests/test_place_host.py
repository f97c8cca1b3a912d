"""The host statement of place recognition (L.scan_descriptor, L.place_distance, L.place_select: lidarslam_amd/csrc/host/lsa_place.cpp
over lsa_scan_descriptor.h) against an independent float64 numpy statement written here, known answers, and the selection
against brute force.  No device."""
import math

import numpy as np
import pytest

SHAPES = [(1, 1), (3, 7), (20, 60), (32, 120)]
MIN_RANGE, MAX_RANGE, OFFSET = 1.5, 61.5, 2.0
EPS = 2.0 ** -23


def bound(rings, sectors):
    """worst-case rounding of the fixed float order on cosines of magnitude <= 1: `rings` products and sums, one division,
    `sectors` sums, one division"""
    return (rings + sectors + 8) * EPS


def params(rings, sectors, **kw):
    return dict(rings=rings, sectors=sectors, min_range=MIN_RANGE, max_range=MAX_RANGE, height_offset=OFFSET, **kw)


# ---- the independent statement ---------------------------------------------------------------------------------------------
def np_cells(xyz, rings, sectors):
    """(ring, sector) coordinates as float64, before the floor, and who takes part"""
    x, y = xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)
    r = np.sqrt(x * x + y * y)
    ok = ~np.isnan(xyz).any(axis=1) & (r >= MIN_RANGE) & (r < MAX_RANGE)
    ring = (r - MIN_RANGE) / (MAX_RANGE - MIN_RANGE) * rings
    sector = (np.arctan2(y, x) + np.pi) / (2 * np.pi) * sectors
    return ring, sector, ok


def np_descriptor(xyz, rings, sectors):
    ring, sector, ok = np_cells(xyz, rings, sectors)
    cells = np.zeros((rings, sectors))
    for i in np.flatnonzero(ok):
        a, b = min(rings - 1, int(ring[i])), min(sectors - 1, max(0, int(sector[i])))
        v = float(xyz[i, 2]) + OFFSET
        if v > cells[a, b]:
            cells[a, b] = v
    return cells, np.sqrt((cells * cells).sum(axis=0))


def np_distances(q, nq, c, nc, min_common):
    """d_s for every shift"""
    rings, sectors = q.shape
    out = np.ones(sectors)
    for s in range(sectors):
        total, cnt = 0.0, 0
        for j in range(sectors):
            k = (j + s) % sectors
            if nq[j] > 0 and nc[k] > 0:
                total += float(q[:, j] @ c[:, k]) / (nq[j] * nc[k])
                cnt += 1
        if cnt >= min_common:
            out[s] = 1.0 - total / cnt
    return out


def polar_cloud(rng, rings, sectors, n):
    """n points in polar form, each in a cell of its own choice and well inside it; heights that float addition keeps exact"""
    ring = rng.integers(0, rings, n)
    sector = rng.integers(0, sectors, n)
    fr, fs = rng.uniform(0.1, 0.9, n), rng.uniform(0.1, 0.9, n)
    z = rng.integers(-3 * 1024, 12 * 1024, n) / 1024.0
    return ring, sector, fr, fs, z


def to_xyz(ring, sector, fr, fs, z, rings, sectors, turn=0):
    """turn: the whole cloud turned about z by that many sectors (exactly: the sector index moves)"""
    r = MIN_RANGE + (ring + fr) / rings * (MAX_RANGE - MIN_RANGE)
    theta = -np.pi + (((sector + turn) % sectors) + fs) / sectors * 2 * np.pi
    return np.column_stack([r * np.cos(theta), r * np.sin(theta), z]).astype(np.float32)


def assert_inside_cells(xyz, rings, sectors):
    """every point at least 1e-6 of a cell's width away from every ring and sector border"""
    ring, sector, ok = np_cells(xyz, rings, sectors)
    assert ok.all()
    for v in (ring, sector):
        f = v - np.floor(v)
        assert np.all((f >= 1e-6) & (f <= 1 - 1e-6))


# what the seeds below give, counted by the numpy statement alone (asserted, so a change of the generator shows):
# (query, candidate) pairs whose best shift leads the runner-up by more than twice the bound, and neighbours in the
# ranking that far apart.  1 x 1 has one shift (every pair decided) and one cosine, 1: all its distances tie.
DECIDED = {(1, 1): (6, 0), (3, 7): (6, 5), (20, 60): (6, 5), (32, 120): (6, 5)}
SEEDS = {(1, 1): 11, (3, 7): 12, (20, 60): 13, (32, 120): 14}


@pytest.mark.parametrize("rings,sectors", SHAPES)
def test_host_statement_follows_the_numpy_statement(L, rings, sectors):
    rng = np.random.default_rng(SEEDS[(rings, sectors)])
    p = params(rings, sectors)
    b = bound(rings, sectors)
    n = 40 * rings
    base = polar_cloud(rng, rings, sectors, n)
    clouds = [to_xyz(*base, rings, sectors)]
    turns = [0, 1 % sectors, 2 % sectors, 5 % sectors, (sectors - 1) % sectors, 3 % sectors]
    for k, turn in enumerate(turns):  # the query turned, with k tenths of its points replaced by others
        other = polar_cloud(rng, rings, sectors, n)
        swap = rng.permutation(n)[: (k * n) // 10]
        mixed = [a.copy() for a in base]
        for a, o in zip(mixed, other):
            a[swap] = o[swap]
        clouds.append(to_xyz(*mixed, rings, sectors, turn=turn))
    host, ref = [], []
    for xyz in clouds:
        assert_inside_cells(xyz, rings, sectors)
        d = L.scan_descriptor(xyz, **p)
        cells, norms = np_descriptor(xyz, rings, sectors)
        assert d.dtype == np.float32 and d.size == rings * sectors + sectors
        assert np.array_equal(cells.astype(np.float32).astype(np.float64), cells)  # the heights are exact in float
        assert np.array_equal(d[: rings * sectors].reshape(rings, sectors).astype(np.float64), cells)
        assert np.all(np.abs(d[rings * sectors:] - norms) <= b * norms)
        host.append(d)
        ref.append((cells, norms))
    min_common = max(1, sectors // 4)
    decided_shift, got_d, want_d = 0, [], []
    for c in range(1, len(clouds)):
        ds = np_distances(*ref[0], *ref[c], min_common)
        best = int(np.argmin(ds))
        gd, gs = L.place_distance(host[0], host[c], **p)
        assert abs(float(gd) - ds[best]) <= b, (c, gd, ds[best])
        runner_up = np.partition(ds, 1)[1] if sectors > 1 else np.inf
        if runner_up - ds[best] > 2 * b:
            decided_shift += 1
            assert gs == best, (c, gs, best)
            if n <= rings * sectors:  # (where the cells are not taken several times over, the turn is recognised)
                assert best == turns[c - 1]
        got_d.append(gd)
        want_d.append(ds[best])
    # the ranking, through the selection with every gate off
    m = len(clouds)
    P = np.tile(np.eye(4), (m, 1, 1))
    got = [f for f, _, _, _ in L.place_select(got_d, np.zeros(m - 1, np.int32), P, np.arange(m), m - 1, sectors=sectors, min_travelled=0.0,
                                              exclusion_half_window=0, capacity=m - 1)]
    order = sorted(range(m - 1), key=lambda i: (want_d[i], i))
    assert sorted(got) == list(range(m - 1))
    decided_rank = 0
    for a, b_ in zip(order, order[1:]):
        if want_d[b_] - want_d[a] > 2 * b:
            decided_rank += 1
            assert got.index(a) < got.index(b_)
    print("decided by the numpy statement:", (rings, sectors), (decided_shift, decided_rank), "distances", [float(d) for d in want_d])
    assert (decided_shift, decided_rank) == DECIDED[(rings, sectors)]


# ---- known answers ---------------------------------------------------------------------------------------------------------
def test_empty_cloud(L):
    p = params(20, 60)
    empty = L.scan_descriptor(np.zeros((0, 3), np.float32), **p)
    assert empty.size == 1260 and not empty.any()
    rng = np.random.default_rng(5)
    full = L.scan_descriptor(to_xyz(*polar_cloud(rng, 20, 60, 500), 20, 60), **p)
    for a, b in [(empty, full), (full, empty), (empty, empty)]:
        assert L.place_distance(a, b, **p) == (np.float32(1.0), 0)


def test_one_point_in_a_known_cell(L):
    p = params(20, 60)
    # r = 1.5 + 3 * 7.5 = 24 m: ring 7 of 20 over [1.5, 61.5); the angle 100 degrees: sector (100 + 180) / 6 = 46
    a = np.deg2rad(100.0)
    d = L.scan_descriptor(np.array([[24.0 * np.cos(a), 24.0 * np.sin(a), 1.5]], np.float32), **p)
    cells = d[:1200].reshape(20, 60)
    assert cells[7, 46] == 3.5 and np.count_nonzero(cells) == 1
    assert d[1200 + 46] == 3.5 and np.count_nonzero(d[1200:]) == 1
    # at or below -height_offset the cell holds 0; out of range, or NaN: no part
    for xyz in ([[10, 0, -2.0]], [[10, 0, -7.0]], [[0.5, 0, 1]], [[61.5, 0, 1]], [[100, 0, 1]], [[np.nan, 0, 1]], [[3, np.nan, 1]], [[3, 0, np.nan]]):
        assert not L.scan_descriptor(np.array(xyz, np.float32), **p).any(), xyz
    # the largest height of a cell, whatever the order
    pts = np.array([[10, 1, 0.5], [10, 1.1, 2.5], [10.1, 1, -1.0]], np.float32)
    for order in ([0, 1, 2], [2, 1, 0], [1, 0, 2]):
        assert L.scan_descriptor(pts[order], **p).max() == 4.5


def test_parameters_out_of_limits(L):
    xyz = np.zeros((1, 3), np.float32)
    for bad in (dict(rings=0), dict(rings=33), dict(sectors=0), dict(sectors=121), dict(type_mask=0), dict(type_mask=8), dict(max_range=0.0), dict(min_range=80.0),
                dict(max_range=float("nan")), dict(max_range=float("inf")), dict(height_offset=float("nan")), dict(height_offset=float("-inf"))):
        with pytest.raises(L.LsaError) as e:
            L.scan_descriptor(xyz, **bad)
        assert e.value.code == L.E_ARG, bad
    assert L.PlaceParams().min_common_sectors == 15 and L.PlaceParams(sectors=7).min_common_sectors == 1 and L.PlaceParams(sectors=120).min_common_sectors == 30


def columns(L, rings, sectors, occupied, rng):
    """a descriptor with exactly these sectors occupied, made of points"""
    n = 4 * len(occupied)
    ring, _, fr, fs, z = polar_cloud(rng, rings, sectors, n)
    sector = np.repeat(np.array(occupied), 4)
    return L.scan_descriptor(to_xyz(ring, sector, fr, fs, np.abs(z) + 0.5, rings, sectors), **params(rings, sectors))


def test_min_common_sectors(L):
    rng = np.random.default_rng(6)
    a = columns(L, 20, 60, list(range(0, 14)), rng)
    assert np.count_nonzero(a[1200:]) == 14
    assert L.place_distance(a, a, **params(20, 60)) == (np.float32(1.0), 0)  # 14 in common at best, 15 wanted
    d, s = L.place_distance(a, a, **params(20, 60, min_common_sectors=14))
    assert s == 0 and abs(d) <= bound(20, 60)
    d, s = L.place_distance(a, a, **params(20, 60, min_common_sectors=1))  # one column in common may do: the best of all shifts
    assert d <= bound(20, 60)


def test_rolled_copy_gives_its_shift(L):
    rng = np.random.default_rng(7)
    for rings, sectors in SHAPES[1:]:
        p = params(rings, sectors)
        a = L.scan_descriptor(to_xyz(*polar_cloud(rng, rings, sectors, 30 * rings), rings, sectors), **p)
        cells, norms = a[: rings * sectors].reshape(rings, sectors), a[rings * sectors:]
        for s in (0, 1, 3, sectors - 1):
            rolled = np.concatenate([np.roll(cells, s, axis=1).ravel(), np.roll(norms, s)])  # column j of a is column j + s of the copy
            d, got = L.place_distance(a, rolled, **p)
            assert got == s and abs(d) <= bound(rings, sectors), (rings, sectors, s, got, d)


def test_a_tie_gives_the_lowest_shift(L):
    rng = np.random.default_rng(8)
    p = params(20, 60)
    ring, _, fr, fs, z = polar_cloud(rng, 20, 60, 5)
    # the same five points in every third sector: the shifts 0, 3, 6, ... tie
    cloud = np.vstack([to_xyz(ring, np.full(5, j), fr, np.full(5, 0.5), np.abs(z) + 1, 20, 60) for j in range(0, 60, 3)])
    a = L.scan_descriptor(cloud, **p)
    cells = a[:1200].reshape(20, 60)
    assert all(np.array_equal(cells[:, 0], cells[:, j]) for j in range(0, 60, 3)) and np.count_nonzero(a[1200:]) == 20
    for s in (0, 3, 30, 57):
        rolled = np.concatenate([np.roll(cells, s, axis=1).ravel(), np.roll(a[1200:], s)])
        assert L.place_distance(a, rolled, **p)[1] == 0
    rolled = np.concatenate([np.roll(cells, 2, axis=1).ravel(), np.roll(a[1200:], 2)])
    assert L.place_distance(a, rolled, **p)[1] == 2  # 2, 5, 8, ... tie


def test_the_sign_of_the_yaw(L):
    """The candidate's cloud is the query's turned by +3 sectors about z -- the query was taken at the candidate's place with
    the base turned by +3 sectors, so everything appears 3 sectors earlier to it: shift 3, yaw +3 * 2 pi / sectors."""
    rng = np.random.default_rng(9)
    for rings, sectors in SHAPES[1:]:
        p = params(rings, sectors)
        ring, sector, _, _, z = polar_cloud(rng, rings, sectors, 25 * rings)
        half = np.full(ring.size, 0.5)  # cell centres
        query = to_xyz(ring, sector, half, half, z, rings, sectors)
        psi = 3 * 2 * np.pi / sectors
        R = np.array([[np.cos(psi), -np.sin(psi), 0], [np.sin(psi), np.cos(psi), 0], [0, 0, 1]])
        candidate = (query.astype(np.float64) @ R.T).astype(np.float32)
        dq, dc = L.scan_descriptor(query, **p), L.scan_descriptor(candidate, **p)
        d, s = L.place_distance(dq, dc, **p)
        assert s == 3 and abs(d) <= bound(rings, sectors)
        m = 2
        P = np.tile(np.eye(4), (m, 1, 1))
        (frame, _, shift, yaw), = L.place_select([d], [s], P, [0.0, 1.0], 1, sectors=sectors, min_travelled=0.0, capacity=1)
        assert (frame, shift) == (0, 3) and yaw == 3 * 2 * math.pi / sectors
    # wrapped to (-pi, pi]
    P = np.tile(np.eye(4), (2, 1, 1))
    assert L.place_select([0.5], [30], P, [0.0, 1.0], 1, sectors=60, min_travelled=0.0, capacity=1)[0][3] == 30 * 2 * math.pi / 60
    assert L.place_select([0.5], [31], P, [0.0, 1.0], 1, sectors=60, min_travelled=0.0, capacity=1)[0][3] == 31 * 2 * math.pi / 60 - 2 * math.pi
    assert L.place_select([0.5], [59], P, [0.0, 1.0], 1, sectors=60, min_travelled=0.0, capacity=1)[0][3] < 0


# ---- the selection against brute force ---------------------------------------------------------------------------------------
def brute_select(distance, shift, P, query, sectors, min_travelled, max_distance, max_descriptor_distance, window, capacity):
    pos = P[:, :3, 3]
    step = [0.0] + [float(np.sqrt(((pos[i] - pos[i - 1]) ** 2).sum())) for i in range(1, query + 1)]
    travelled = [0.0]
    for i in range(1, query + 1):
        travelled.append(travelled[-1] + step[i])
    ok = []
    for i in range(query):
        if not (travelled[query] - travelled[i] >= min_travelled):
            continue
        if max_distance > 0 and not (float(np.sqrt(((pos[i] - pos[query]) ** 2).sum())) <= max_distance):
            continue
        if max_descriptor_distance > 0 and not (float(distance[i]) <= max_descriptor_distance):
            continue
        ok.append(i)
    ok.sort(key=lambda i: (distance[i], i))
    out = []
    while ok and len(out) < capacity:
        i = ok[0]
        yaw = shift[i] * 2 * math.pi / sectors
        out.append((i, distance[i], int(shift[i]), yaw - 2 * math.pi if yaw > math.pi else yaw))
        ok = [j for j in ok if abs(j - i) > window]
    return out


def test_select_follows_brute_force(L):
    rng = np.random.default_rng(10)
    n = 60
    # a loop: out along x, back near the start
    P = np.tile(np.eye(4), (n, 1, 1))
    a = np.linspace(0, 2 * np.pi, n)
    P[:, 0, 3], P[:, 1, 3], P[:, 2, 3] = 20 * np.sin(a), 20 * (1 - np.cos(a)), rng.normal(0, 0.05, n)
    t = 0.1 * np.arange(n)
    distance = rng.uniform(0.05, 0.9, n).astype(np.float32)
    distance[[3, 4, 10, 11, 12, 40]] = np.float32(0.05)  # ties on distance: the lower index, and the window around it
    distance[[0, 58]] = np.float32(0.01)                  # the best at both ends of the log
    shift = rng.integers(0, 60, n).astype(np.int32)
    cases = 0
    for query in (n - 1, 30, 1, 0):
        for min_travelled in (0.0, 10.0, 60.0, 1000.0):
            for max_distance in (0.0, 8.0, 25.0):
                for gate in (0.0, 0.05, 0.3):
                    for window in (0, 1, 5, 100):
                        for capacity in (0, 1, 4, 100):
                            got = L.place_select(distance[:query], shift[:query], P, t, query, sectors=60, min_travelled=min_travelled, max_distance=max_distance,
                                                 max_descriptor_distance=gate, exclusion_half_window=window, capacity=capacity)
                            want = brute_select(distance, shift, P, query, 60, min_travelled, max_distance, gate, window, capacity)
                            assert got == want, (query, min_travelled, max_distance, gate, window, capacity, got, want)
                            cases += len(want) > 0
    assert cases > 300
    # what the cases are meant to show, on the brute-force statement
    first = brute_select(distance, shift, P, n - 1, 60, 0.0, 0.0, 0.0, 1, 4)
    assert [c[0] for c in first] == [0, 58, 3, 10]  # 1 and 57 fall to the window at either end, 4 to 3's, 11 to 10's
    assert brute_select(distance, shift, P, n - 1, 60, 10.0, 0.0, 0.0, 1, 1)[0][0] == 0  # frame 58 is not 10 m back
    for bad in (dict(query=n), dict(query=-1), dict(min_travelled=-1.0), dict(exclusion_half_window=-1), dict(sectors=0), dict(capacity=-1)):
        kw = {**dict(query=n - 1, sectors=60, min_travelled=0.0, exclusion_half_window=0, capacity=3), **bad}
        query = kw.pop("query")
        with pytest.raises(L.LsaError) as e:
            L.place_select(distance, shift, P, t, query, **kw)
        assert e.value.code == L.E_ARG, bad
