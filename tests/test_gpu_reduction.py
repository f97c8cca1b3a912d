"""The 29 normal-equation sums of k_accumulate (lsa_accumulate) and k_lm_solve (lsa_solve_device) at forced launch shapes,
against the exactly rounded sum of the very per-block values the kernels add, within the per-entry bound derived in
tests/reduction_cases.py (d read from the code for the shape that ran), and bit for bit where the sum is exact.

Every case uploads its residual blocks (lsa_upload_match), forces its shape (lsa_debug_set) and checks from
lsa_solve_device_shape / lsa_accumulate_shape that this shape is the one that ran."""
import numpy as np
import pytest

import reduction_cases as RC
from conftest import bits

pytestmark = pytest.mark.gpu

KNOBS = ("lm_blocks", "lm_records", "lm_cache", "accum_blocks", "mailbox_check")
CAP = 99  # lm_cache above any capacity: the knob clamps it to what the probe found

# k_lm_solve: (nb, total, lm_cache).  nb in {1, 7, 8, 9, 63, 64}; totals at nb * 512 * p and +-1 for p = 1, 2, 3, 5;
# cslots in {0, 1, capacity}; per_thread in {1, cslots, cslots + 1, >= 4}
LM_SHAPES = [(1, 512, CAP), (1, 513, CAP), (1, 2561, CAP), (7, 7167, 1), (8, 12288, 0), (9, 4609, 1), (9, 23039, 0), (63, 64513, CAP),
             (64, 32767, 1), (64, 163840, 1), (8, 8193, 1), (7, 3584, 0)]
# k_accumulate: (accum_blocks, total); per_thread 6, 3, 2, 3, 1
ACC_SHAPES = [(1, 1281), (2, 1536), (3, 1535), (96, 49153), (256, 65535)]


@pytest.fixture(scope="module")
def rctx(L):
    ctx = L.Context(0)
    yield ctx
    ctx.close()


@pytest.fixture
def ctx(rctx):
    yield rctx
    for k in KNOBS:  # no other test sees a forced shape
        rctx.debug_set(k, -1)


def upload(ctx, rs):
    for t in range(3):
        ctx.upload_match(t, rs.status[t], rs.records[t], rs.sat[t])


@pytest.fixture(scope="module")
def capacity(rctx):
    """the LDS layers the solve kernel gets: the knob at its most (clamped to the probe's capacity), 6 residual blocks
    per thread at one workgroup"""
    upload(rctx, RC.exact_set(3, RC.split(2561, 0)))
    rctx.debug_set("lm_blocks", 1)
    rctx.debug_set("lm_records", 256)
    rctx.debug_set("lm_cache", CAP)
    try:
        rctx.solve_device(7, np.zeros(6), max_iter=0)
        nb, per_thread, cslots, total = rctx.solve_device_shape()
    finally:
        for k in KNOBS:
            rctx.debug_set(k, -1)
    print(f"k_lm_solve LDS cache capacity: {cslots} layers")
    assert (nb, per_thread, total) == (1, 6, 2561)
    return cslots


def test_the_lds_cache_capacity_launches(ctx, O, capacity):
    """the capacity the context probed (lm_cache_capacity) is at least one layer, and a launch that uses all of it runs
    and gives the exact sums"""
    assert capacity >= 1, "no LDS layer for the residual blocks"
    rs = RC.exact_set(4, RC.split(2561, 1), g_zero=True)
    upload(ctx, rs)
    force_lm(ctx, 1, CAP)
    r = ctx.solve_device(7, np.zeros(6))
    assert ctx.solve_device_shape() == (1, 6, capacity, 2561)
    assert_exact(solve_sums(r), r.num_matches, RC.Reference(O, rs, np.zeros(6)), "solve at the LDS capacity")
    assert ctx.solve_device_fallbacks() == 0


def force_lm(ctx, nb, cache):
    ctx.debug_set("lm_blocks", nb)
    ctx.debug_set("lm_records", 256)
    ctx.debug_set("lm_cache", cache)


def lm_expected(nb, total, cache, capacity):
    per_thread = -(-total // (nb * 512))
    return (nb, per_thread, min(per_thread, capacity if cache == CAP else cache), total)


def acc_expected(blocks, total):
    return (blocks, -(-total // (blocks * 256)), 0, total)


def solve_sums(r):
    return RC.sums_of(r.cost, r.g, r.H)


def check_bound(ref, S, d, what):
    bad = ref.violations(S, d)
    err = np.abs(np.asarray(S) - ref.sums)
    print(f"{what}: d {d}, worst err / bound {np.max(err / np.maximum(ref.bound(d), 1e-300)):.3g}")
    assert bad.size == 0, f"{what}: entries {bad.tolist()} outside the bound: dev {np.asarray(S)[bad]} ref {ref.sums[bad]} bound {ref.bound(d)[bad]}"


def assert_exact(S, count, ref, what):
    assert count == ref.count, f"{what}: count {count} != {ref.count}"
    diff = np.flatnonzero(bits(np.asarray(S, np.float64) + 0.0) != bits(ref.sums))
    assert diff.size == 0, f"{what}: entries {diff.tolist()} not the exact sums: dev {np.asarray(S)[diff]} exact {ref.sums[diff]}"


# ---------------------------------------------------------------------------------------------------------------- upload
def test_upload_match_round_trip(ctx):
    rs = RC.rejected(RC.random_set(11, (700, 0, 5000), 1), RC.reject_rows(5700, (700, 0, 5000), 512, "single"))
    upload(ctx, rs)
    for t in (0, 2):
        st, w, rec = ctx.match_results(t, n=rs.counts[t])
        ok = rs.status[t] == 0
        assert np.array_equal(st, rs.status[t])
        assert np.array_equal(bits(rec[ok]), bits(rs.records[t][ok])) and not np.any(rec[~ok])
    # a larger set grows the buffer (the outgrown one is retired); the knobs restore what the context was created with
    big = RC.exact_set(12, (40000, 0, 0))
    upload(ctx, big)
    st, w, rec = ctx.match_results(0, n=40000)
    assert np.array_equal(bits(rec), bits(big.records[0]))
    ctx.debug_set("lm_blocks", 3)
    ctx.solve_device(7, np.zeros(6), max_iter=0)
    assert ctx.solve_device_shape()[0] == 3
    ctx.debug_set("lm_blocks", -1)
    ctx.solve_device(7, np.zeros(6), max_iter=0)
    assert ctx.solve_device_shape()[0] == min(-(-40000 // 512), 64)


# ------------------------------------------------------------------------------------------------------------ k_accumulate
@pytest.mark.parametrize("i,shape", list(enumerate(ACC_SHAPES)), ids=[f"ab{b}-n{n}" for b, n in ACC_SHAPES])
def test_accumulate_exact(ctx, O, i, shape):
    blocks, total = shape
    rs = RC.exact_set(100 + i, RC.split(total, i))
    upload(ctx, rs)
    ctx.debug_set("accum_blocks", blocks)
    ref = RC.Reference(O, rs, np.zeros(6))
    c, g, H, n = ctx.accumulate(7, np.zeros(6))
    assert ctx.accumulate_shape() == acc_expected(blocks, total)
    S = RC.sums_of(c, g, H)
    assert_exact(S, n, ref, f"accumulate EXACT {shape}")
    # two launches, the cost without the Jacobian, and the mailbox checked against the device's own fold: the same bits
    c2, g2, H2, n2 = ctx.accumulate(7, np.zeros(6))
    assert np.array_equal(bits(RC.sums_of(c2, g2, H2)), bits(S)) and n2 == n
    cj = ctx.accumulate(7, np.zeros(6), jac=False)
    assert bits(np.float64(cj[0])) == bits(np.float64(c)) and cj[3] == n
    ctx.debug_set("mailbox_check", 1)
    cm, gm, Hm, nm = ctx.accumulate(7, np.zeros(6))  # raises when mailbox and device fold disagree
    assert np.array_equal(bits(RC.sums_of(cm, gm, Hm)), bits(S)) and nm == n


@pytest.mark.parametrize("family", ["RANDOM", "CANCEL"])
@pytest.mark.parametrize("i,shape", list(enumerate(ACC_SHAPES)), ids=[f"ab{b}-n{n}" for b, n in ACC_SHAPES])
def test_accumulate_within_the_bound(ctx, O, i, shape, family):
    blocks, total = shape
    rs = (RC.random_set(200 + i, RC.split(total, i), i) if family == "RANDOM" else RC.cancel_set(300 + i, RC.split(total, i), i))
    upload(ctx, rs)
    ctx.debug_set("accum_blocks", blocks)
    ctx.debug_set("mailbox_check", i % 2)
    for w in rs.points:
        ref = RC.Reference(O, rs, w)
        c, g, H, n = ctx.accumulate(7, w)
        shp = ctx.accumulate_shape()
        assert shp == acc_expected(blocks, total)
        assert n == ref.count
        d = RC.depth_accum(blocks, shp[1])
        assert d <= RC.D_WIDE
        check_bound(ref, RC.sums_of(c, g, H), d, f"accumulate {rs} {shape} at {w}")
        cj = ctx.accumulate(7, w, jac=False)
        assert bits(np.float64(cj[0])) == bits(np.float64(c))


@pytest.mark.parametrize("pattern", RC.REJECT_PATTERNS)
@pytest.mark.parametrize("i,shape", [(0, ACC_SHAPES[0]), (3, ACC_SHAPES[3])], ids=["ab1", "ab96"])
def test_accumulate_never_reads_rejected_rows(ctx, O, i, shape, pattern):
    blocks, total = shape
    ctx.debug_set("accum_blocks", blocks)
    for j, rs in enumerate((RC.exact_set(400 + i, RC.split(total, i)), RC.random_set(500 + i, RC.split(total, i + 1), i))):
        mask = RC.reject_rows(total, rs.counts, blocks * 256, pattern)
        bad, zero = RC.rejected(rs, mask), RC.rejected(rs, mask, zero_payload=True)
        w = rs.points[-1]
        upload(ctx, zero)
        b = ctx.accumulate(7, w)
        upload(ctx, bad)
        a = ctx.accumulate(7, w)
        assert ctx.accumulate_shape() == acc_expected(blocks, total)
        Sa, Sb = RC.sums_of(*a[:3]), RC.sums_of(*b[:3])
        assert np.array_equal(bits(Sa), bits(Sb)) and a[3] == b[3] == rs.total - int(mask.sum())
        ref = RC.Reference(O, bad, w)
        if bad.family.startswith("EXACT"):
            assert_exact(Sa, a[3], ref, f"accumulate {bad} {pattern}")
        else:
            check_bound(ref, Sa, RC.depth_accum(blocks, ctx.accumulate_shape()[1]), f"accumulate {bad} {pattern}")


# -------------------------------------------------------------------------------------------------------------- k_lm_solve
LM_IDS = [f"nb{nb}-n{n}-c{c}" for nb, n, c in LM_SHAPES]


@pytest.mark.parametrize("i,shape", list(enumerate(LM_SHAPES)), ids=LM_IDS)
def test_solve_exact(ctx, O, capacity, i, shape):
    nb, total, cache = shape
    want = lm_expected(nb, total, cache, capacity)
    force_lm(ctx, nb, cache)
    # g = 0: the solve stops at iteration 0 (gradient tolerance) and hands back the exact sums at the start point
    rs = RC.exact_set(600 + i, RC.split(total, i), g_zero=True)
    upload(ctx, rs)
    ref = RC.Reference(O, rs, np.zeros(6))
    assert not np.any(ref.sums[1:7])
    r = ctx.solve_device(7, np.zeros(6))
    assert ctx.solve_device_shape() == want
    assert (r.termination, r.num_iterations, r.skipped) == (2, 0, 0)
    assert_exact(solve_sums(r), r.num_matches, ref, f"solve EXACT g = 0 {shape}")
    assert bits(np.float64(r.initial_cost)) == bits(ref.sums[0]) and list(r.pose) == [0.0] * 6
    # g != 0: the cost at the start point is exact
    rs = RC.exact_set(700 + i, RC.split(total, i + 1))
    upload(ctx, rs)
    ref = RC.Reference(O, rs, np.zeros(6))
    r = ctx.solve_device(7, np.zeros(6))
    assert ctx.solve_device_shape() == want
    assert bits(np.float64(r.initial_cost)) == bits(ref.sums[0]) and r.num_matches == ref.count
    assert ctx.solve_device_fallbacks() == 0


@pytest.mark.parametrize("family", ["RANDOM", "CANCEL"])
@pytest.mark.parametrize("i,shape", list(enumerate(LM_SHAPES)), ids=LM_IDS)
def test_solve_within_the_bound(ctx, O, capacity, i, shape, family):
    nb, total, cache = shape
    want = lm_expected(nb, total, cache, capacity)
    rs = (RC.random_set(800 + i, RC.split(total, i), i) if family == "RANDOM" else RC.cancel_set(900 + i, RC.split(total, i), i))
    upload(ctx, rs)
    force_lm(ctx, nb, cache)
    r = ctx.solve_device(7, rs.prior)
    shp = ctx.solve_device_shape()
    assert shp == want
    d = RC.depth_lm(nb, shp[1])
    assert not r.skipped and r.num_evaluations >= 1
    ref0 = RC.Reference(O, rs, rs.prior)
    bound0 = ref0.bound(d)[0]
    print(f"solve {rs} {shape}: initial cost err / bound {abs(r.initial_cost - ref0.sums[0]) / bound0:.3g}")
    assert abs(r.initial_cost - ref0.sums[0]) <= bound0
    # the sums it returns are those at the pose it returns, bit for bit that pose
    pose = np.array(r.pose)
    ref = RC.Reference(O, rs, pose)
    assert r.num_matches == ref.count
    check_bound(ref, solve_sums(r), d, f"solve {rs} {shape} at the returned pose")
    assert ctx.solve_device_fallbacks() == 0


@pytest.mark.parametrize("i,shape", list(enumerate(LM_SHAPES)), ids=LM_IDS)
def test_one_launch_equals_the_host_driven_loop_at_forced_shapes(ctx, capacity, i, shape):
    """the tolerance of tests/test_gpu_match.py::test_one_launch_solve_equals_the_host_driven_loop (lsa_solve reports
    no termination code: the step counts stand for it)"""
    nb, total, cache = shape
    rs = RC.random_set(1000 + i, RC.split(total, i), i)
    upload(ctx, rs)
    force_lm(ctx, nb, cache)
    ctx.debug_set("accum_blocks", ACC_SHAPES[i % len(ACC_SHAPES)][0])
    r = ctx.solve_device(7, rs.prior, max_iter=15)
    assert ctx.solve_device_shape() == lm_expected(nb, total, cache, capacity)
    # (the host-driven loop starts from the pose matrix of the same parameters)
    pose_h, summ, costs = ctx.solve(7, RC.pose_matrix(rs.prior), max_iter=15)
    assert (r.num_successful_steps, r.num_unsuccessful_steps, r.num_iterations, r.num_evaluations) == tuple(int(v) for v in summ)
    assert np.abs(RC.pose_matrix(np.array(r.pose)) - pose_h).max() < 1e-9, (list(r.pose), pose_h)
    assert ctx.solve_device_fallbacks() == 0


@pytest.mark.parametrize("pattern", RC.REJECT_PATTERNS)
@pytest.mark.parametrize("i,shape", [(1, LM_SHAPES[1]), (5, LM_SHAPES[5]), (9, LM_SHAPES[9])], ids=[LM_IDS[1], LM_IDS[5], LM_IDS[9]])
def test_solve_never_reads_rejected_rows(ctx, O, capacity, i, shape, pattern):
    nb, total, cache = shape
    force_lm(ctx, nb, cache)
    for rs in (RC.exact_set(1100 + i, RC.split(total, i), g_zero=True), RC.random_set(1200 + i, RC.split(total, i + 1), i)):
        mask = RC.reject_rows(total, rs.counts, nb * 512, pattern)
        bad, zero = RC.rejected(rs, mask), RC.rejected(rs, mask, zero_payload=True)
        upload(ctx, zero)
        b = ctx.solve_device(7, rs.prior)
        upload(ctx, bad)
        a = ctx.solve_device(7, rs.prior)
        assert ctx.solve_device_shape() == lm_expected(nb, total, cache, capacity)
        assert a.num_matches == b.num_matches == rs.total - int(mask.sum())
        assert list(a.pose) == list(b.pose) and (a.termination, a.num_evaluations) == (b.termination, b.num_evaluations)
        assert np.array_equal(bits(solve_sums(a)), bits(solve_sums(b)))
        assert bits(np.float64(a.initial_cost)) == bits(np.float64(b.initial_cost))
        if bad.family.startswith("EXACT"):
            ref = RC.Reference(O, bad, np.zeros(6))
            assert a.num_matches == ref.count and bits(np.float64(a.initial_cost)) == bits(ref.sums[0])
    assert ctx.solve_device_fallbacks() == 0
