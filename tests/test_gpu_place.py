"""Place recognition on the keypoint log: k_log_describe, the log's descriptor store, k_place_search and
Slam.recognize_place on top of them.

The reference is the host statement (L.scan_descriptor, L.place_distance, L.place_select), which compiles the same
definition (lidarslam_amd/csrc/lsa_scan_descriptor.h) and which tests/test_place_host.py holds to an independent numpy
statement: device and host must agree byte for byte -- cells, norms, distances, shifts, candidates."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# rings, sectors, the other parameters
SHAPES = [
    (1, 1, {}),
    (3, 7, dict(min_range=2.5, max_range=50.0, height_offset=1.25)),
    (20, 60, {}),
    (32, 120, dict(height_offset=-1.0)),
]
SIZES = [0, 1, 63, 64, 65, 257, 3000]


def points(L, xyz):
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(xyz.shape[0], L.POINT_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["w"] = 1.0
    return p


def three_ways(pts):
    """a frame: the points dealt out to the three keypoint types in turn"""
    return [pts[k::3].copy() for k in range(3)]


def host_descriptor(L, frame, type_mask=3, **params):
    chosen = [frame[k] for k in range(3) if (type_mask >> k) & 1]
    return L.scan_descriptor(np.concatenate(chosen), type_mask=type_mask, **params)


def border_points(rng):
    """points exactly on ring borders of every shape used, on the four axes, at the origin, with negative zeros"""
    out = []
    for rings, _, extra in SHAPES:
        lo, hi = extra.get("min_range", 0.0), extra.get("max_range", 80.0)
        for k in range(rings + 1):
            r = np.float32(k * (hi - lo) / rings + lo)
            for x, y in [(r, 0.0), (-r, 0.0), (0.0, r), (0.0, -r), (r, -0.0), (-r, -0.0), (-0.0, r)]:
                out.append((x, y, rng.uniform(-3, 3)))
    for z in (-0.0, 0.0, 1.0, -2.0, -1.25, 1.0000001):
        out += [(0.0, 0.0, z), (-0.0, -0.0, z), (0.0, -0.0, z), (-0.0, 0.0, z)]
    # sector borders: the angles k * 2 pi / sectors as float arithmetic gives them, at a few radii
    for _, sectors, _ in SHAPES:
        for k in range(sectors):
            a = -np.pi + k * 2 * np.pi / sectors
            for r in (1.0, 7.5, 33.0):
                out.append((r * np.cos(a), r * np.sin(a), rng.uniform(-3, 3)))
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def describe_log(L):
    rng = np.random.default_rng(20261019)
    frames = []
    for n in SIZES:  # x, y in +-70: radii up to 99, a good part beyond max_range
        frames.append(three_ways(points(L, np.column_stack([rng.uniform(-70, 70, n), rng.uniform(-70, 70, n), rng.uniform(-4, 6, n)]))))
    one_cell = np.column_stack([10.0 + rng.uniform(0, 0.01, 3000), 10.0 + rng.uniform(0, 0.01, 3000), rng.uniform(-5, 5, 3000)])
    frames.append(three_ways(points(L, one_cell)))
    beyond = np.column_stack([rng.uniform(80, 200, 257) * rng.choice([-1, 1], 257), rng.uniform(80, 200, 257), rng.uniform(-4, 6, 257)])
    frames.append(three_ways(points(L, beyond)))
    nan = np.column_stack([rng.uniform(-40, 40, 300), rng.uniform(-40, 40, 300), rng.uniform(-4, 6, 300)])
    nan[0::4, 0] = np.nan
    nan[1::4, 1] = np.nan
    nan[2::4, 2] = np.nan
    frames.append(three_ways(points(L, nan)))
    all_nan = nan.copy()
    all_nan[:, 2] = np.nan
    frames.append(three_ways(points(L, all_nan)))
    frames.append(three_ways(points(L, border_points(rng))))
    frames.append([points(L, np.zeros((0, 3))), points(L, [[5, 5, 1]]), points(L, np.zeros((0, 3)))])  # one type only
    return frames


@pytest.mark.parametrize("rings,sectors,extra", SHAPES)
def test_descriptors_equal_the_host_statement(L, gpu_ctx, describe_log, rings, sectors, extra):
    ctx = gpu_ctx
    ctx.kplog_clear()
    try:
        for fr in describe_log:
            ctx.kplog_append_points(fr)
        n = len(describe_log)
        occupied = 0
        for mask in range(1, 8):
            p = dict(rings=rings, sectors=sectors, type_mask=mask, **extra)
            assert ctx.kplog_describe(0, n - 1, **p) == n  # the mask changed: everything again
            got = ctx.kplog_descriptors(0, n - 1, **p)
            for i, fr in enumerate(describe_log):
                want = host_descriptor(L, fr, **p)
                assert got[i].tobytes() == want.tobytes(), (rings, sectors, mask, i, np.flatnonzero(got[i].view(np.uint32) != want.view(np.uint32))[:8])
                occupied += int((want > 0).sum())
        assert occupied > 0
        # all points beyond max_range, and all points NaN: nothing but zeros
        p = dict(rings=rings, sectors=sectors, type_mask=7, **extra)
        got = ctx.kplog_descriptors(0, n - 1, **p)
        assert not got[0].any() and not got[len(SIZES) + 1].any() and not got[len(SIZES) + 3].any()
    finally:
        ctx.kplog_clear()


def test_the_store_follows_the_log(L, gpu_ctx, describe_log):
    ctx = gpu_ctx
    ctx.kplog_clear()
    p = dict(rings=20, sectors=60)
    q = dict(rings=20, sectors=60, height_offset=3.0)
    try:
        log = [describe_log[i] for i in (6, 5, 4, 3, 9)]
        for fr in log:
            ctx.kplog_append_points(fr)
        want = [host_descriptor(L, fr, **p) for fr in log]
        # a range call describes its range only, a second one what is left
        assert ctx.kplog_describe(1, 2, **p) == 2 and ctx.kplog_described() == 2
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_descriptors(0, 2, **p)
        assert e.value.code == L.E_STATE
        assert ctx.kplog_describe(1, 2, **p) == 0 and ctx.kplog_described() == 0
        assert ctx.kplog_describe(0, 4, **p) == 3
        assert ctx.kplog_descriptors(0, 4, **p).tobytes() == np.stack(want).tobytes()
        # pop the front, append, describe again: the survivors are as they were and where they belong, the new one is right
        ctx.kplog_pop_front()
        ctx.kplog_pop_front()
        for i in (7, 11):
            ctx.kplog_append_points(describe_log[i])
            log.append(describe_log[i])
            want.append(host_descriptor(L, describe_log[i], **p))
        log, want = log[2:], want[2:]
        assert ctx.kplog_size() == 5
        assert ctx.kplog_describe(0, 4, **p) == 2
        assert ctx.kplog_descriptors(0, 4, **p).tobytes() == np.stack(want).tobytes()
        # a search describes what it needs and no more
        d, s = ctx.kplog_place_search(4, 0, 3, **p)
        assert ctx.kplog_described() == 0
        # the ring of slots goes round (64 slots at this size): after 2 + 61 pops the five frames sit in slots 63, 0, 1, 2, 3
        for turn in range(61):
            ctx.kplog_pop_front()
            fr = describe_log[(turn * 5) % len(describe_log)]
            ctx.kplog_append_points(fr)
            log = log[1:] + [fr]
            want = want[1:] + [host_descriptor(L, fr, **p)]
            assert ctx.kplog_describe(0, 4, **p) == 1
        assert ctx.kplog_descriptors(0, 4, **p).tobytes() == np.stack(want).tobytes()
        # the store grows with the log and keeps what it holds (the move unwraps the ring)
        for i in range(80):
            fr = describe_log[i % len(describe_log)]
            ctx.kplog_append_points(fr)
            log.append(fr)
        assert ctx.kplog_describe(0, len(log) - 1, **p) == 80
        got = ctx.kplog_descriptors(0, len(log) - 1, **p)
        assert got[:5].tobytes() == np.stack(want).tobytes()
        assert all(got[i].tobytes() == host_descriptor(L, log[i], **p).tobytes() for i in range(5, len(log)))
        # a parameter change recomputes everything
        assert ctx.kplog_describe(0, 4, **q) == 5
        assert ctx.kplog_descriptors(0, 4, **q).tobytes() == np.stack([host_descriptor(L, fr, **q) for fr in log[:5]]).tobytes()
        with pytest.raises(L.LsaError):
            ctx.kplog_descriptors(0, 5, **q)
        assert ctx.kplog_describe(0, 4, **p) == 5
        # kplog_clear empties it
        ctx.kplog_clear()
        ctx.kplog_append_points(log[0])
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_descriptors(0, 0, **p)
        assert e.value.code == L.E_STATE
        assert ctx.kplog_describe(0, 0, **p) == 1
    finally:
        ctx.kplog_clear()


# ---- the search --------------------------------------------------------------------------------------------------------------
NCAND = 300
QUERIES = {"full": NCAND, "empty": NCAND + 1, "periodic": NCAND + 2, "sparse": NCAND + 3}


def ring_cloud(rng, sectors_used, total_sectors=60, rings=(10.0, 30.0, 50.0), heights=None):
    """points at cell centres of a 60-sector layout, in the given sectors: the same heights in every sector unless given"""
    out = []
    for j in sectors_used:
        a = -np.pi + (j + 0.5) * 2 * np.pi / total_sectors
        for i, r in enumerate(rings):
            z = (1.0 + i) if heights is None else heights[(j, i)]
            out.append((r * np.cos(a), r * np.sin(a), z))
    return np.array(out, np.float32)


@pytest.fixture(scope="module")
def search_log(L):
    """300 candidates and four queries: small frames, every case of the search among them"""
    rng = np.random.default_rng(777)

    def scene(n):
        return np.column_stack([rng.uniform(-60, 60, n), rng.uniform(-60, 60, n), rng.uniform(-3, 8, n)])

    base = scene(400)
    periodic = ring_cloud(rng, range(60))          # every sector alike: every shift gives the same distance
    half = ring_cloud(rng, range(0, 60, 2))        # period 2: the even shifts tie
    sparse = ring_cloud(rng, range(0, 10), heights={(j, i): rng.uniform(0.5, 5) for j in range(10) for i in range(3)})
    frames = []
    for c in range(NCAND):
        kind = c % 10
        if kind == 0:
            xyz = base                                # identical to the query "full"
        elif kind == 1:
            xyz = np.zeros((0, 3))                    # an empty candidate
        elif kind == 2:                               # the query turned about z by whole sectors of the 60-sector shape
            a = (c // 10 % 60) * 2 * np.pi / 60
            R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            xyz = base @ R.T
        elif kind == 3:
            xyz = periodic
        elif kind == 4:
            xyz = half
        elif kind == 5:
            xyz = sparse                              # 10 of 60 sectors: fewer in common than min_common_sectors = 15
        elif kind == 6:
            xyz = np.vstack([base[: 200], scene(100)])
        else:
            xyz = scene(int(rng.integers(1, 300)))
        frames.append(three_ways(points(L, xyz)))
    frames.append(three_ways(points(L, base)))                 # QUERIES["full"]
    frames.append(three_ways(points(L, np.zeros((0, 3)))))     # "empty"
    frames.append(three_ways(points(L, periodic)))             # "periodic"
    frames.append(three_ways(points(L, sparse)))               # "sparse"
    return frames


@pytest.fixture(scope="module")
def search_expected(L, search_log):
    """per shape and query the host statement's table over all candidates: computed once"""
    made = {}

    def get(rings, sectors, extra, query):
        key = (rings, sectors, query)
        if key not in made:
            p = dict(rings=rings, sectors=sectors, type_mask=7, **extra)
            desc = [host_descriptor(L, fr, **p) for fr in search_log]
            table = [L.place_distance(desc[QUERIES[query]], desc[c], **p) for c in range(NCAND)]
            made[key] = (np.array([t[0] for t in table], np.float32), np.array([t[1] for t in table], np.int32))
        return made[key]

    return get


@pytest.fixture(scope="module")
def search_ctx(L, gpu_ctx, search_log):
    ctx = gpu_ctx
    ctx.kplog_clear()
    for fr in search_log:
        ctx.kplog_append_points(fr)
    yield ctx
    ctx.debug_set("place_max_blocks", 0)
    ctx.debug_set("place_untiled", 0)
    ctx.kplog_clear()


@pytest.mark.parametrize("rings,sectors,extra", SHAPES)
def test_search_table_equals_the_host_statement(L, search_ctx, search_expected, rings, sectors, extra):
    ctx = search_ctx
    p = dict(rings=rings, sectors=sectors, type_mask=7, **extra)
    for query in QUERIES:
        want_d, want_s = search_expected(rings, sectors, extra, query)
        # 300 candidates: more workgroups than the chip has CUs; 7 workgroups: every one strides over 42 or 43 candidates;
        # short ranges from a first > 0 (lengths 3 and 5: no multiple of four or of two pairs, should the search ever run as a row
        # of k_place_search_rows), the first and the last frame alone; all of it under both settings of "place_untiled", which
        # k_place_search does not read
        for first, last, blocks in [(0, NCAND - 1, 0), (0, NCAND - 1, 7), (17, 17, 0), (29, 30, 0), (101, 165, 0), (101, 165, 64), (7, 9, 0), (40, 44, 0), (0, 0, 0),
                                    (NCAND - 1, NCAND - 1, 0)]:
            for untiled in (0, 1):
                ctx.debug_set("place_max_blocks", blocks)
                ctx.debug_set("place_untiled", untiled)
                d, s = ctx.kplog_place_search(QUERIES[query], first, last, **p)
                assert d.size == last - first + 1
                assert d.tobytes() == want_d[first:last + 1].tobytes(), (query, first, last, blocks, untiled, np.flatnonzero(d != want_d[first:last + 1])[:8])
                assert np.array_equal(s, want_s[first:last + 1]), (query, first, last, blocks, untiled, np.flatnonzero(s != want_s[first:last + 1])[:8])
    ctx.debug_set("place_max_blocks", 0)
    ctx.debug_set("place_untiled", 0)


@pytest.mark.parametrize("rings,sectors,extra", SHAPES[1:3])
def test_search_across_the_wrap_of_the_store(L, search_log, rings, sectors, extra):
    """70 frames described: a store of 105 slots (half as much again as the log, lsa_place.hip: ensure_store), frame i in slot
    i.  40 popped from the front, 40 appended: 70 <= 105, so the store stays and its head is slot 40 -- frame i in slot
    (40 + i) % 105, the frames 65..69 in slots 0..4, past the wrap, the query (69) among them.  A context of its own: the
    store of another test would be larger and not wrap."""
    p = dict(rings=rings, sectors=sectors, type_mask=7, **extra)
    ctx = L.Context(0)
    try:
        for fr in search_log[:70]:
            ctx.kplog_append_points(fr)
        assert ctx.kplog_describe(0, 69, **p) == 70
        for _ in range(40):
            ctx.kplog_pop_front()
        for fr in search_log[100:140]:
            ctx.kplog_append_points(fr)
        log = search_log[40:70] + search_log[100:140]
        assert ctx.kplog_size() == len(log) == 70
        d, s = ctx.kplog_place_search(69, 0, 68, **p)
        assert ctx.kplog_described() == 40  # the survivors kept their descriptors, the store was not made anew
        desc = [host_descriptor(L, fr, **p) for fr in log]
        assert ctx.kplog_descriptors(0, 69, **p).tobytes() == np.stack(desc).tobytes()
        table = [L.place_distance(desc[69], desc[c], **p) for c in range(69)]
        want_d, want_s = np.array([t[0] for t in table], np.float32), np.array([t[1] for t in table], np.int32)
        assert d.tobytes() == want_d.tobytes(), np.flatnonzero(d != want_d)[:8]
        assert np.array_equal(s, want_s), np.flatnonzero(s != want_s)[:8]
        assert len(set(want_d.tolist())) > 10  # (the table is no constant)
    finally:
        ctx.close()


def test_search_cases_are_what_they_are_meant_to_be(L, search_ctx, search_expected):
    """conditions on the host table alone (20 x 60): the cases the search is held to are really in it"""
    rings, sectors, extra = SHAPES[2]
    d, s = search_expected(rings, sectors, extra, "full")
    kinds = np.arange(NCAND) % 10
    assert np.all(d[kinds == 0] <= 1e-6) and np.all(s[kinds == 0] == 0)       # identical to the query
    assert np.all(d[kinds == 1] == 1.0) and np.all(s[kinds == 1] == 0)        # an empty candidate
    turned = np.flatnonzero(kinds == 2)
    assert np.all(d[turned] < 0.2)                                             # turned copies are recognised, at their shift
    assert np.array_equal(s[turned], (turned // 10) % 60)
    assert len(set(s[turned].tolist())) >= 25
    d, s = search_expected(rings, sectors, extra, "empty")
    assert np.all(d == 1.0) and np.all(s == 0)                                 # an empty query
    d, s = search_expected(rings, sectors, extra, "periodic")
    assert np.all(s[kinds == 3] == 0) and np.all(d[kinds == 3] <= 1e-6)       # every shift ties: the lowest
    assert np.all(s[kinds == 4] == 0) and np.all(d[kinds == 4] <= 1e-6)       # (half the columns in common under every shift)
    d, s = search_expected(rings, sectors, extra, "sparse")
    assert np.all(d[kinds == 5] == 1.0)                                        # 10 sectors in common < 15
    p = dict(rings=rings, sectors=sectors, type_mask=7, min_common_sectors=10)
    got_d, got_s = search_ctx.kplog_place_search(QUERIES["sparse"], 5, 5, **p)
    assert got_d[0] <= 1e-6 and got_s[0] == 0                                  # ... and enough once 10 will do


def test_refusals_leave_the_outputs_alone(L, search_ctx):
    ctx = search_ctx
    n = ctx.kplog_size()
    out = (np.full(8, 7.5, np.float32), np.full(8, -9, np.int32))
    bad = [
        dict(query=0, first=-1, last=2), dict(query=0, first=3, last=2), dict(query=0, first=0, last=n), dict(query=n, first=0, last=2), dict(query=-1, first=0, last=2),
        dict(query=0, first=0, last=2, rings=0), dict(query=0, first=0, last=2, rings=33), dict(query=0, first=0, last=2, sectors=0), dict(query=0, first=0, last=2, sectors=121),
        dict(query=0, first=0, last=2, type_mask=0), dict(query=0, first=0, last=2, type_mask=8), dict(query=0, first=0, last=2, min_range=80.0),
        dict(query=0, first=0, last=2, max_range=float("nan")), dict(query=0, first=0, last=2, height_offset=float("inf")),
    ]
    for case in bad:
        case = dict(case)
        query, first, last = case.pop("query"), case.pop("first"), case.pop("last")
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_place_search(query, first, last, out=out, **case)
        assert e.value.code == L.E_ARG, case
        assert np.all(out[0] == 7.5) and np.all(out[1] == -9)
        if "rings" in case or "sectors" in case or "type_mask" in case or "min_range" in case or "max_range" in case or "height_offset" in case:
            with pytest.raises(L.LsaError) as e:
                ctx.kplog_describe(first, last, **case)
            assert e.value.code == L.E_ARG, case
    with pytest.raises(L.LsaError) as e:
        ctx.kplog_describe(0, n)
    assert e.value.code == L.E_ARG


def test_a_stopped_log_refuses(L, describe_log):
    ctx = L.Context(0)
    try:
        ctx.debug_set("kplog_chunk_kib", 16)
        ctx.kplog_append_points(describe_log[3])
        ctx.kplog_append_points(describe_log[4])
        ctx.debug_set("kplog_fail_alloc", 1)
        with pytest.raises(L.LsaError):
            ctx.kplog_append_points(describe_log[6])  # needs a chunk of its own, which cannot be had
        assert ctx.kplog_stopped()
        out = (np.full(2, 7.5, np.float32), np.full(2, -9, np.int32))
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_place_search(1, 0, 1, out=out)
        assert e.value.code == L.E_STATE and np.all(out[0] == 7.5) and np.all(out[1] == -9)
        with pytest.raises(L.LsaError) as e:
            ctx.kplog_describe(0, 1)
        assert e.value.code == L.E_STATE
    finally:
        ctx.debug_set("kplog_fail_alloc", 0)
        ctx.close()


# ---- Slam.recognize_place ----------------------------------------------------------------------------------------------------
MODEL, SEED, FORWARD = 16, 1000, 12


@pytest.fixture(scope="module")
def frames(L):
    return [L.synth_frame(MODEL, SEED, f) for f in range(FORWARD)]


@pytest.fixture(scope="module")
def revisit(L, frames):
    """frames 0..11 forward, then the clouds 10..0 again with increasing stamps: the vehicle backs up over its own track"""
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    period = frames[1][1] - frames[0][1]
    order = list(range(FORWARD)) + list(range(FORWARD - 2, -1, -1))
    for f, c in enumerate(order):
        s.add_frame(frames[c][0], frames[0][1] + f * period, f)
    P, t, _ = s.trajectory()
    assert P.shape[0] == len(order) == s.logged_frames()
    yield s, P, t, order
    s.close()


def Rz(yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    return T


def host_recognize(L, s, P, t, query, capacity, search, **descriptor):
    mask = descriptor.get("type_mask", 3)
    desc = [L.scan_descriptor(np.concatenate([s.logged_keypoints(i, k) for k in range(3) if (mask >> k) & 1]), **descriptor) for i in range(query + 1)]
    table = [L.place_distance(desc[query], desc[i], **descriptor) for i in range(query)]
    return L.place_select([d for d, _ in table], [sh for _, sh in table], P, t, query, sectors=descriptor.get("sectors", 60), capacity=capacity, **search)


def test_recognize_place_on_a_revisit(L, revisit):
    s, P, t, order = revisit
    q = len(order) - 1
    # the trajectory returns to where it began (a condition on the construction, not on the feature)
    back = np.linalg.norm(P[q][:3, 3] - P[0][:3, 3])
    way = np.linalg.norm(np.diff(P[:, :3, 3], axis=0), axis=1).sum()
    print("revisit: way", way, "back to", back, "of the start")
    assert way > 4.0 and back < 0.5
    for search, descriptor in [
        (dict(min_travelled=2.0, max_distance=0.0, exclusion_half_window=2), {}),
        (dict(min_travelled=2.0, max_distance=1.0, exclusion_half_window=0), {}),
        (dict(min_travelled=0.0, max_distance=0.0, max_descriptor_distance=0.2, exclusion_half_window=1), dict(rings=32, sectors=120, type_mask=7)),
        (dict(min_travelled=1.0, exclusion_half_window=3), dict(rings=3, sectors=7, min_range=2.5, max_range=50.0, type_mask=2)),
    ]:
        for query in (q, q - 5, 3):
            for capacity in (0, 1, 4):
                got = s.recognize_place(query, capacity=capacity, **search, **descriptor)
                want = host_recognize(L, s, P, t, query, capacity, search, **descriptor)
                assert got == want, (search, descriptor, query, capacity, got, want)
                assert len(got) <= capacity
    assert s.recognize_place(0) == []
    # the last frame saw what frame 0 saw; the position gate is off
    got = s.recognize_place(q, capacity=3, min_travelled=2.0, max_distance=0.0, exclusion_half_window=2)
    print("candidates of the last frame:", got)
    frame, distance, shift, yaw = got[0]
    assert abs(order[frame] - order[q]) <= 1 and frame <= 1, got
    assert distance < 0.2 and abs(yaw) <= 2 * np.pi / 60 + 1e-12
    res = s.register_logged_frames(q, frame, L.LoopClosureParams(revisited_half_window=2), P[frame] @ Rz(yaw))
    print("registered: status", res.status, "iterations", res.iterations, "relative translation", res.relative[:3, 3])
    assert res.status == 0


def test_recognize_place_refusals(L, revisit, frames):
    s, P, t, order = revisit
    for query, params in [(len(order), {}), (-1, {}), (5, dict(rings=0)), (5, dict(sectors=121)), (5, dict(type_mask=0)), (5, dict(min_travelled=-1.0)),
                          (5, dict(exclusion_half_window=-1)), (5, dict(max_range=-1.0))]:
        with pytest.raises(L.LsaError) as e:
            s.recognize_place(query, **params)
        assert e.value.code == L.E_ARG, (query, params)
    off = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    for f in range(3):
        off.add_frame(frames[f][0], frames[f][1], f)
    with pytest.raises(L.LsaError) as e:
        off.recognize_place(2, min_travelled=0.0)
    assert e.value.code == L.E_STATE and "LoggingTimeout" in str(e.value)
    off.set_param("LoggingTimeout", -1)
    for f in range(3, 5):
        off.add_frame(frames[f][0], frames[f][1], f)
    with pytest.raises(L.LsaError) as e:
        off.recognize_place(4, min_travelled=0.0)
    assert e.value.code == L.E_STATE and "does not cover" in str(e.value)
    off.close()


# ---- the frame path does not notice ------------------------------------------------------------------------------------------
def snapshot(L, s):
    P, t, cov = s.trajectory()
    return (s.world_transform().tobytes(), s.covariance().tobytes(), [s.map(k).tobytes() for k in (L.EDGE, L.PLANE)],
            [s.target_submap(k).tobytes() for k in (L.EDGE, L.PLANE)], P.tobytes(), t.tobytes(), cov.tobytes(), s.logged_frames(),
            s.get_param("NbrFrameProcessed"))


@pytest.mark.parametrize("on_device", [1, 0])
def test_the_frame_path_does_not_notice_a_recognition(L, frames, on_device):
    def run(recognize):
        s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, MapsOnDevice=on_device)
        shots = []
        for f, (pts, stamp) in enumerate(frames):
            s.add_frame(pts, stamp, f)
            if f in (6, 9):
                # (both runs read the same state through the same getters the same number of times: the recognitions and
                #  the refused call are the only difference between them)
                before = snapshot(L, s)
                if recognize:
                    found = s.recognize_place(f, min_travelled=1.0, exclusion_half_window=1)
                    assert len(found) >= 1
                    s.recognize_place(f - 1, min_travelled=0.0, rings=32, sectors=120, type_mask=7)
                    with pytest.raises(L.LsaError):
                        s.recognize_place(f + 1)
                assert snapshot(L, s) == before
            if f >= 7:
                shots.append(snapshot(L, s))
        assert s.get_param("DeviceSolveFallbacks") == 0
        s.close()
        return shots

    assert run(True) == run(False)
