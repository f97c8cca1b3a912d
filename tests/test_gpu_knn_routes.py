"""The exact kNN search against brute-force neighbour LISTS on every route it can take (tests/knn_cases.py): the two-launch
form of lsa_match_fused.hip and the staged form of lsa_match_staged.hip leave their lists in memory (lsa_download_knn), the
one-launch form is held to the two-launch form's status, weights and records bit for bit, all three to the oracle's, and the
counters of LSA_ROUTE_STATS confirm that every named case took the route its construction derives.

cnt as stored: min(k, m) neighbours found; -1 (planes and blobs) the k-th neighbour is proven beyond the rejection distance,
accepted only where the reference's k-th squared distance, as double, exceeds max_neighbors_distance^2, with status
NEIGHBORS_TOO_FAR; -2 (two-launch form) settled by the whole-target search, the lists then hold the answer and their number
equals lsa_match_slow_queries.  The staged form answers such queries in its second kernel, which rewrites the count: it
never stores -2, and its lsa_match_slow_queries counts hand-overs between its kernels, another quantity: on the anchored
cases it is held to the number the reference's k-th distances give (knn_cases.staged_handovers), and where every query
ends in the whole-target search, so must lsa_match_exhaustive_queries.

The staged form is swept over 8, 16 and 32 lanes and 2 and 3 rounds: lsa_set_knn_rounds accepts nothing else (1 is
LSA_E_ARG), so these are all the round counts there are.

Far cases: the exits by the counts (first three shells, a later shell) are counted in route[3], which must equal the number of
-1 entries; the exit after the first scan is taken behind the counters, so its case asserts route[3] == 0 WHILE -1 entries
exist -- the only way the two are told apart today."""
import numpy as np
import pytest

import knn_cases as K
from conftest import bits

pytestmark = pytest.mark.gpu

TOO_FAR = 3  # LSA_MATCH_NEIGHBORS_TOO_FAR
INT_MAX = 0x7FFFFFFF


def _context(L, stats):
    mp = pytest.MonkeyPatch()
    if stats:
        mp.setenv("LSA_ROUTE_STATS", "1")
    else:
        mp.delenv("LSA_ROUTE_STATS", raising=False)
    try:
        return L.Context(0)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def stats_ctx(L):
    ctx = _context(L, True)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def plain_ctx(L):
    ctx = _context(L, False)
    yield ctx
    ctx.close()


_ORACLE = {}


def oracle_match(O, case):
    if case.name not in _ORACLE:
        _ORACLE[case.name] = O.match(case.queries, case.target, case.ktype, case.mp, np.eye(4) if case.pose is None else case.pose)
    return _ORACLE[case.name]


def run(ctx, L, case, form, lanes=None, rounds=None):
    t = case.ktype
    ctx.set_fused_match(form)
    if form == 0:
        ctx._check(ctx.L.lsa_set_knn_lanes(ctx.h, t, lanes or (16, 8, 8)[t]), "lsa_set_knn_lanes")
        ctx._check(ctx.L.lsa_set_knn_rounds(ctx.h, t, rounds or 2), "lsa_set_knn_rounds")
    ctx.set_keypoints(L.SET_WORKING, t, case.queries)
    ctx.set_target(t, case.target, cell=case.cell)
    hist = ctx.match(t, L.SET_WORKING, case.mp, np.eye(4) if case.pose is None else case.pose)
    st, w, rec = ctx.match_results(t, L.SET_WORKING)
    idx, d2, cnt = ctx.knn_lists(t, capacity=case.queries.size)
    return dict(hist=hist, st=st, w=w, rec=rec, idx=idx, d2=d2, cnt=cnt, slow=ctx.slow_queries(), stats=ctx.route_stats(t), rounds=rounds or 2)


def assert_lists(case, r, O, form, what=""):
    ridx, rd2 = K.reference(case, O)
    nq, kk, k = case.queries.size, ridx.shape[1], case.k
    idx, d2, cnt = r["idx"], r["d2"], r["cnt"]
    assert idx.shape == (nq, K.KNN_MAX) and d2.shape == (nq, K.KNN_MAX) and cnt.shape == (nq,), what
    print(f"{case.name} form {form} {what}: cnt -1 x {(cnt == -1).sum()}, -2 x {(cnt == -2).sum()}, slow {r['slow']}, stats {r['stats'].tolist()}")
    far, tail = cnt == -1, cnt == -2
    assert np.all(cnt[~far & ~tail] == kk), (what, np.unique(cnt))
    ok = ~far
    bad = np.flatnonzero(ok & np.any(idx[:, :kk] != ridx, axis=1))
    assert bad.size == 0, f"{what}: neighbour indices differ at queries {bad[:8].tolist()}: got {idx[bad[:2], :kk].tolist()} want {ridx[bad[:2]].tolist()}"
    bad = np.flatnonzero(ok & np.any(bits(d2[:, :kk]) != bits(rd2), axis=1))
    assert bad.size == 0, f"{what}: distances differ at queries {bad[:8].tolist()}"
    # behind the neighbours found: nothing, as the header documents it
    assert np.all(idx[ok, kk:k] == INT_MAX) and np.all(np.isposinf(d2[ok, kk:])) and np.all(idx[:, k:] == -1), what
    if far.any():
        assert case.ktype != K.EDGE, what
        assert K.beyond_rejection(case, O)[far].all(), f"{what}: -1 where the k-th neighbour is within the rejection distance"
        assert np.all(r["st"][far] == TOO_FAR), what
    if form == 2:
        assert tail.sum() == r["slow"], (what, tail.sum(), r["slow"])
    else:
        assert not tail.any(), what
        if case.anchored and not case.name.startswith("far_"):
            assert r["slow"] == K.staged_handovers(case, r["rounds"], O), (what, r["slow"])
        if "tail" in case.routes:
            assert r["slow"] == nq and r["stats"][1] == nq, (what, r["stats"][:2].tolist())


def assert_same_match(a, b, what):
    assert a["hist"].tolist() == b["hist"].tolist(), what
    assert np.array_equal(a["st"], b["st"]), (what, np.flatnonzero(a["st"] != b["st"])[:8])
    assert np.array_equal(bits(a["w"]), bits(b["w"])) and np.array_equal(bits(a["rec"]), bits(b["rec"])), what


def assert_routes(case, r):
    nq, tags = case.queries.size, case.routes
    slow, route, far = int(r["stats"][0]), r["stats"][2:8].tolist(), int((r["cnt"] == -1).sum())
    assert slow == r["slow"]
    if "second" in tags:
        assert route[0] == nq
    if "at_once" in tags:
        assert route[0] == 0
    if "shell0" in tags:
        assert route[4] == nq
    if "not_shell0" in tags:
        assert route[4] == 0
    if "beyond2" in tags:
        assert route[1] == nq
    if "within2" in tags:
        assert route[1] == 0
    if "far_counts" in tags:
        assert route[3] == far and 0 < far < nq
    if "far_scan" in tags:
        assert route[3] == 0 and 0 < far < nq
    if "no_far" in tags:
        assert route[3] == 0 and far == 0
    if "tail" in tags:
        assert slow == nq
    if "no_tail" in tags:
        assert slow == 0
    if "all_heavy" in tags:
        assert route[2] > 0 and route[5] == 0
    if "light" in tags:
        assert route[5] > 0
    if case.tags.get("heavy_too"):
        # half of the queries walk 3k candidates with their lanes (at most 3k each): the rest of the candidates counted are
        # the whole-wavefront scans of the other half
        assert route[2] > (nq // 2) * 3 * case.k


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.name)
def test_neighbour_lists_equal_brute_force_on_every_route(stats_ctx, O, L, case):
    two = run(stats_ctx, L, case, 2)
    assert_lists(case, two, O, 2, "two-launch form")
    assert_routes(case, two)
    staged = run(stats_ctx, L, case, 0)
    assert_lists(case, staged, O, 0, "staged form")
    one = run(stats_ctx, L, case, 1)
    assert one["idx"].shape[0] == 0  # by design: the lists never leave the chip
    assert one["stats"].tolist() == two["stats"].tolist(), "the one-launch form takes the same routes"
    assert_same_match(one, two, "one-launch against two-launch form")
    so, wo, ro, ho = oracle_match(O, case)
    ref = dict(hist=ho, st=so, w=wo, rec=ro)
    for name, r in (("one-launch", one), ("two-launch", two), ("staged", staged)):
        assert_same_match(r, ref, f"{name} form against the oracle")


@pytest.mark.parametrize("case", [c for c in K.CASES if c.sweep], ids=lambda c: c.name)
def test_staged_form_at_every_lane_and_round_count(plain_ctx, O, L, case):
    ref = None
    for lanes in (8, 16, 32):
        for rounds in (2, 3):
            r = run(plain_ctx, L, case, 0, lanes, rounds)
            assert_lists(case, r, O, 0, f"staged form, {lanes} lanes, {rounds} rounds")
            ref = ref or r
            assert_same_match(r, ref, f"staged form, {lanes} lanes, {rounds} rounds")
    run(plain_ctx, L, case, 0)  # the defaults back


@pytest.mark.parametrize("name", ["second_scan_sh3_edge16", "heavy_alternating_plane16", "lattice_dup_edge10", "far_later_plane5_d10", "tail_unproven_plane5"])
def test_route_counters_do_not_change_a_result(stats_ctx, plain_ctx, O, L, name):
    case = K.BY_NAME[name]
    for form in (2, 1):
        a, b = run(stats_ctx, L, case, form), run(plain_ctx, L, case, form)
        assert_same_match(a, b, f"form {form}")
        assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(bits(a["d2"]), bits(b["d2"])) and np.array_equal(a["cnt"], b["cnt"])
        assert a["slow"] == b["slow"] and not b["stats"][2:8].any()  # (nothing is counted without LSA_ROUTE_STATS)
        if form == 2:
            assert_lists(case, b, O, 2, "counters off")


@pytest.mark.parametrize("name", ["tail_isolated_edge8", "budget_flat_plane5", "second_scan_sh6_plane16"])
def test_overlap_estimator_nearest_distances(plain_ctx, O, L, name):
    """lsa_overlap searches with the staged kernels at k = 1 (the smallest instantiation, used by nothing else): slot 0 of
    the lists is the brute-force nearest neighbour of every sampled point"""
    case = K.BY_NAME[name]
    tx = K.xyz32(case.target).astype(np.float64)
    rng = np.random.default_rng(3)
    frame = K.points(np.concatenate([rng.uniform(tx.min(0) - 5.0, tx.max(0) + 5.0, (500, 3)), K.xyz32(case.queries).astype(np.float64)]))
    ratio = np.float32(0.5)
    nb = int(np.float32(frame.size) * ratio)
    src = (np.arange(nb, dtype=np.float32) / ratio).astype(np.int64)
    plain_ctx.upload_frame(frame)
    plain_ctx.set_target(L.PLANE, case.target, cell=case.cell)
    got = plain_ctx.overlap(1 << L.PLANE, float(ratio), (0.6, 0.6, 0.6), np.eye(4))
    idx, d2, cnt = plain_ctx.knn_lists(L.PLANE, capacity=nb)
    ridx, rd2 = K.brute_knn(K.xyz32(case.target), K.xyz32(frame[src]), 1)
    assert idx.shape[0] == nb and np.all(cnt == 1)
    assert np.array_equal(bits(d2[:, 0]), bits(rd2[:, 0])) and np.array_equal(idx[:, 0], ridx[:, 0])
    assert np.all(idx[:, 1:] == -1)
    # and the estimate is the mean of the scores of exactly these distances (float sum in another order: to rounding)
    want = np.exp(-rd2[:, 0].astype(np.float64) / (2.0 * (0.6 / 3.0) ** 2)).mean()
    assert abs(got - want) <= 2e-5  # scores are at most 1: a few float32 roundings each, summed in float32
