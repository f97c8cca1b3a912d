"""The list keeping of the exact kNN search (lsa_match_fused.hip: LaneList and group_min by v_min_f64 / v_max_f64 on the keys'
bits, the turns of scan_rows, the second scan) on the cases of tests/knn_list_cases.py: distances 0 and in the f64 denormal
range of the keys, blocks whose candidates end exactly at a turn's edge, the 64-lane scans, and candidates exactly at and one
ulp beyond the k-th distance of the first scan.

The two-launch form leaves its lists in memory (lsa_download_knn): they are held to knn_cases.brute_knn entry for entry, every
query of every case.  The one-launch form (lists never leave the chip) and the staged form (which shares group_min) are held to
the two-launch form's status, weights and records as bit patterns; the staged form's lists to the same brute force.  The
counters of LSA_ROUTE_STATS confirm the route a case was built for."""
import numpy as np
import pytest

import knn_cases as K
import knn_list_cases as C
from conftest import bits

pytestmark = pytest.mark.gpu

INT_MAX = 0x7FFFFFFF


@pytest.fixture(scope="module")
def stats_ctx(L):
    mp = pytest.MonkeyPatch()
    mp.setenv("LSA_ROUTE_STATS", "1")
    try:
        ctx = L.Context(0)
    finally:
        mp.undo()
    yield ctx
    ctx.close()


def run(ctx, L, case, form):
    t = case.ktype
    ctx.set_fused_match(form)
    if form == 0:
        ctx._check(ctx.L.lsa_set_knn_lanes(ctx.h, t, (16, 8, 8)[t]), "lsa_set_knn_lanes")
        ctx._check(ctx.L.lsa_set_knn_rounds(ctx.h, t, 2), "lsa_set_knn_rounds")
    ctx.set_keypoints(L.SET_WORKING, t, case.queries)
    ctx.set_target(t, case.target, cell=case.cell)
    hist = ctx.match(t, L.SET_WORKING, case.mp, np.eye(4))
    st, w, rec = ctx.match_results(t, L.SET_WORKING)
    idx, d2, cnt = ctx.knn_lists(t, capacity=case.queries.size)
    return dict(hist=hist, st=st, w=w, rec=rec, idx=idx, d2=d2, cnt=cnt, slow=ctx.slow_queries(), stats=ctx.route_stats(t))


def assert_lists(case, r, form):
    ridx, rd2 = K.reference(case)
    nq, kk, k = case.queries.size, ridx.shape[1], case.k
    idx, d2, cnt = r["idx"], r["d2"], r["cnt"]
    assert idx.shape == (nq, K.KNN_MAX) and d2.shape == (nq, K.KNN_MAX) and cnt.shape == (nq,)
    tail = cnt == -2
    assert np.all(cnt[~tail] == kk), np.unique(cnt)  # (no rejection distance in these cases: never -1)
    assert int(tail.sum()) == (r["slow"] if form == 2 else 0)
    bad = np.flatnonzero(np.any(idx[:, :kk] != ridx, axis=1))
    assert bad.size == 0, f"form {form}: neighbour indices differ at queries {bad[:8].tolist()}: got {idx[bad[:2], :kk].tolist()} want {ridx[bad[:2]].tolist()}"
    bad = np.flatnonzero(np.any(bits(d2[:, :kk]) != bits(rd2), axis=1))
    assert bad.size == 0, f"form {form}: distance bits differ at queries {bad[:8].tolist()}"
    assert np.all(idx[:, kk:k] == INT_MAX) and np.all(np.isposinf(d2[:, kk:])) and np.all(idx[:, k:] == -1)


def assert_same_match(a, b, what):
    assert a["hist"].tolist() == b["hist"].tolist(), what
    assert np.array_equal(a["st"], b["st"]), (what, np.flatnonzero(a["st"] != b["st"])[:8])
    assert np.array_equal(bits(a["w"]), bits(b["w"])) and np.array_equal(bits(a["rec"]), bits(b["rec"])), what


def assert_routes(case, r):
    nq, tags = case.queries.size, case.routes
    route = r["stats"][2:8].tolist()
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
    if "tail" in tags:
        assert r["slow"] == nq
    if "no_tail" in tags:
        assert r["slow"] == 0
    if "all_heavy" in tags:
        assert route[2] > 0 and route[5] == 0
    if "light" in tags:
        assert route[5] > 0
    assert route[3] == 0


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_lists_equal_brute_force_whatever_the_keys_and_fill_levels(stats_ctx, L, case):
    two = run(stats_ctx, L, case, 2)
    assert_lists(case, two, 2)
    assert_routes(case, two)
    if case.name.startswith("bound_"):
        # said once more in the case's own terms: the mirrored point took the k-th place, the first scan's k-th is gone
        assert np.all(two["idx"][:, case.k - 1] == case.tags["mirror"])
        assert not np.any(two["idx"][:, :case.k] == case.tags["kth"]) and not np.any(two["idx"][:, :case.k] == case.tags["beyond"])
    one = run(stats_ctx, L, case, 1)
    assert one["idx"].shape[0] == 0  # by design: the lists never leave the chip
    assert one["stats"].tolist() == two["stats"].tolist(), "the one-launch form takes the same routes"
    assert_same_match(one, two, "one-launch against two-launch form")
    staged = run(stats_ctx, L, case, 0)
    assert_lists(case, staged, 0)
    assert_same_match(staged, two, "staged against two-launch form")
