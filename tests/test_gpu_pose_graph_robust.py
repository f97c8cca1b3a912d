"""Robust losses in the device pose-graph solver (lidarslam_amd/csrc/lsa_pose_graph.hip: k_pgo_linearize_robust,
k_pgo_linearize_priors_robust, k_pgo_chi2_robust, k_pgo_chi2_priors_robust) held to the host statement: the weighted linearization
bit for bit, the branch borders hit exactly, the solve and its verdicts; the Slam calls on a logged revisit; the example."""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

import pose_graph_cases as PG
import pose_graph_prior_cases as PP
import pose_graph_robust_cases as RC
from conftest import bits, pose_diff
from test_cpp_api import build_example

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))


NAMES = ("e", "blocks", "chi2", "rho", "w")


# ---- the linearization ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257, 3000])
def test_robust_linearization_equals_the_host_twin_bit_for_bit(L, gpu_ctx, m):
    poses, _, edges = PG.edge_count_graph(m)
    E = L.pose_graph_edges(edges)
    chi2 = L.pose_graph_linearize(poses, E)[2]
    c = float(np.sqrt(np.median(chi2)))  # edges on both sides of c2
    last = np.zeros(m, np.uint8)
    last[-1] = 1
    masks = {"all": None, "none": np.zeros(m, np.uint8), "alternating": (np.arange(m) % 2).astype(np.uint8), "last": last}
    for loss in RC.LOSSES:
        rb = L.PoseGraphRobust(edge_loss=loss, edge_scale=c, prior_loss=RC.TUKEY, prior_scale=1.0)
        for name, mask in masks.items():
            host = L.pose_graph_linearize_robust(poses, E, rb, mask=mask)
            dev = L.pose_graph_linearize_robust(poses, E, rb, mask=mask, ctx=gpu_ctx)
            for h, d, what in zip(host, dev, NAMES):
                assert same_bits(h, d), (m, RC.LOSS_NAMES[loss], name, what, np.abs(h - d).max())
            if loss != RC.NONE and name == "all" and m > 1:
                assert (dev[4] < 1.0).any()
            if name == "none":
                assert np.all(dev[4] == 1.0) and same_bits(dev[3], dev[2])


@pytest.mark.parametrize("k", [1, 64, 65, 257])
def test_robust_prior_linearization_equals_the_host_twin_bit_for_bit(L, gpu_ctx, k):
    poses, _, _ = PG.feature_graph()
    priors, O = PP.feature_priors(k)
    R = L.pose_graph_priors(priors)
    chi2 = L.pose_graph_linearize_priors(poses, R, O)[2]
    c = float(np.sqrt(np.median(chi2)))
    for loss in RC.LOSSES:
        rb = L.PoseGraphRobust(prior_loss=loss, prior_scale=c, edge_loss=RC.HUBER, edge_scale=1.0)
        host = L.pose_graph_linearize_priors_robust(poses, R, rb, O)
        dev = L.pose_graph_linearize_priors_robust(poses, R, rb, O, ctx=gpu_ctx)
        for h, d, what in zip(host, dev, NAMES):
            assert same_bits(h, d), (k, RC.LOSS_NAMES[loss], what, np.abs(h - d).max())
        assert same_bits(dev[1], dev[4][:, None] * L.pose_graph_linearize_priors(poses, R, O)[1])


def test_the_branch_borders_hit_exactly(L, gpu_ctx):
    """Identity poses, relative = a pure translation (d, 0, 0), information I: chi2 = d d with no rounding but the product's.
    c = 2: d = 2 is s == c2, the inner branch; its neighbours on either side; 0; a denormal chi2; 1e16."""
    ds = [2.0, float(np.nextafter(2.0, 3.0)), float(np.nextafter(2.0, 1.0)), 0.0, 1e-160, 1e8]
    poses = np.array([np.eye(4), np.eye(4)])
    edges = []
    for d in ds:
        Z = np.eye(4)
        Z[0, 3] = d
        edges.append((0, 1, Z, np.eye(6)))
    s = np.array([d * d for d in ds])
    assert s[0] == 4.0 and s[1] > 4.0 > s[2] and 0.0 < s[4] < 2.3e-308
    for loss in RC.LOSSES:
        rb = L.PoseGraphRobust(edge_loss=loss, edge_scale=2.0)
        host = L.pose_graph_linearize_robust(poses, edges, rb)
        dev = L.pose_graph_linearize_robust(poses, edges, rb, ctx=gpu_ctx)
        for h, d, what in zip(host, dev, NAMES):
            assert same_bits(h, d), (RC.LOSS_NAMES[loss], what)
        assert same_bits(dev[2], s)
        rho, w = L.pose_graph_robust_rho(loss, 2.0, s)
        assert same_bits(dev[3], rho) and same_bits(dev[4], w)
        if loss == RC.HUBER:
            assert dev[3][0] == 4.0 and dev[4][0] == 1.0 and dev[4][1] <= 1.0 and dev[3][2] == s[2] and dev[4][5] == 2.0 / 1e8
        if loss == RC.TUKEY:
            assert dev[4][0] == 0.0 and dev[3][0] == 4.0 / 3.0 and dev[4][1] == 0.0 and dev[3][1] == 4.0 / 3.0 and 0.0 < dev[4][2] < 1e-30
            assert dev[4][3] == 1.0 and dev[3][3] == 0.0 and dev[4][4] == 1.0 and dev[4][5] == 0.0


# ---- no loss: the solver as it was ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["circle64", "gps64"])
def test_no_loss_gives_the_bits_of_the_existing_entries(L, gpu_ctx, graph):
    if graph == "circle64":
        (poses, fixed, edges), priors, O = PG.circle_graph(64)[:3], None, None
    else:
        _, poses, fixed, edges, priors, O, _ = PP.gps_case(64, 4)
    ref, rref = gpu_ctx.pose_graph_solve(poses, fixed, edges, priors=priors, offset=O)
    m = len(edges)
    for rb, mask in ((L.PoseGraphRobust(), None), (L.PoseGraphRobust(edge_scale=0.5), (np.arange(m) % 2).astype(np.uint8)),
                     (L.PoseGraphRobust(edge_loss=RC.TUKEY, edge_scale=1.0), np.zeros(m, np.uint8))):
        out, r, ev, pv = L.pose_graph_solve_robust(poses, fixed, edges, rb, mask=mask, ctx=gpu_ctx, priors=priors, offset=O)
        assert same_bits(out, ref)
        for name in ("initial_cost", "final_cost", "largest_step", "final_lambda"):
            assert same_bits(getattr(r, name), getattr(rref, name)), name
        assert (r.iterations, r.accepted_steps, r.rejected_steps, r.pcg_iterations, r.termination) == (
            rref.iterations, rref.accepted_steps, rref.rejected_steps, rref.pcg_iterations, rref.termination)
        assert same_bits(ev[:, 0], L.pose_graph_linearize(out, edges)[2]) and np.all(ev[:, 1] == 1.0)
        if priors is not None:
            assert same_bits(pv[:, 0], L.pose_graph_linearize_priors(out, priors, O)[2]) and np.all(pv[:, 1] == 1.0)


def test_refusals_write_nothing(L, gpu_ctx):
    start, fixed, edges, mask, priors, O, _, _ = RC.robust_gps_graph(16, 3, (1,))
    P = np.ascontiguousarray(start.reshape(-1, 16))
    E, R = L.pose_graph_edges(edges), L.pose_graph_priors(priors)
    Om = np.ascontiguousarray(O.reshape(16))
    p = L.PoseGraphParams()
    for bad in (dict(edge_loss=4), dict(prior_loss=-1), dict(edge_loss=1, edge_scale=0.0), dict(prior_loss=3, prior_scale=float("nan"))):
        rb = L.PoseGraphRobust(**bad)
        out, ev, pv = np.full_like(P, -7.0), np.full((E.size, 2), -7.0), np.full((R.size, 2), -7.0)
        r = L.PoseGraphResultStruct()
        rc = L.lib().lsa_pgo_solve_robust(gpu_ctx.h, L.ptr(P), P.shape[0], L.ptr(fixed), L.ptr(E), E.size, L.ptr(mask), L.ptr(R), R.size, L.ptr(Om), C.byref(p), C.byref(rb),
                                          L.ptr(out), C.byref(r), L.ptr(ev), L.ptr(pv))
        assert rc == L.E_ARG and np.all(out == -7.0) and np.all(ev == -7.0) and np.all(pv == -7.0)
        with pytest.raises(L.LsaError) as e:
            L.pose_graph_linearize_robust(start, edges, rb, mask=mask, ctx=gpu_ctx)
        assert e.value.code == L.E_ARG
    with pytest.raises(L.LsaError) as e:
        L.pose_graph_solve_robust(start, fixed, edges, L.PoseGraphRobust(edge_loss=RC.TUKEY), mask=mask[:-1], ctx=gpu_ctx, priors=priors, offset=O)
    assert e.value.code == L.E_ARG


# ---- the solve --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_case(n):
    """five true and two false loops, a fix at every eighth pose with two of them 50 m off, pose 0 held: with every pose free the
    fixes of 0.5 m alone hold the track as a whole, so loosely that a cost of 3e4 (the plain solve, which takes the outliers at full
    weight) no longer resolves the last 1e-7 m -- the host statement run with the other preconditioner shows it (1e-7 m apart)"""
    return RC.robust_gps_graph(n, 8, (1, 4), True, True, RC.FALSE_OFFSET, True)


@pytest.mark.parametrize("loss", RC.LOSSES)
@pytest.mark.parametrize("n", [64, 257, 1000])
def test_robust_solve_against_the_host_statement(L, gpu_ctx, n, loss):
    """1e-7 m / 1e-6 rad, the project's tolerance for the device against the host statement.  Both run to the step
    tolerance (cost_tolerance 0): with the default relative decrease of 1e-13 the PLAIN solve of these graphs -- no loss, two
    loops and two fixes 50 m off dragging at a cost of 3e4 -- stops 1e-5 m short of its minimum, the host statement itself shows,
    and where exactly it stops is then a matter of the last bits of the cost."""
    start, fixed, edges, mask, priors, O, bad, false = solve_case(n)
    E, R = L.pose_graph_edges(edges), L.pose_graph_priors(priors)
    rb = L.PoseGraphRobust(edge_loss=loss, edge_scale=RC.SCALE, prior_loss=loss, prior_scale=RC.SCALE)
    p = L.PoseGraphParams(cost_tolerance=0.0, max_iterations=200)
    host, hres, hev, hpv = L.pose_graph_solve_robust(start, fixed, E, rb, mask=mask, params=p, priors=R, offset=O)
    # the input conditions, on the host statement: no outcome hangs on the path
    c2 = RC.SCALE**2
    loops = mask.astype(bool)
    chi0 = L.pose_graph_linearize(start, E)[2]
    pchi0 = L.pose_graph_linearize_priors(start, R, O)[2]
    assert int(false.sum()) == 2 and int((loops & ~false).sum()) == 5 and int(bad.sum()) == 2
    assert chi0[loops & ~false].max() < c2 / 4 and pchi0[~bad].max() < c2 / 4
    assert chi0[false].min() > 100 * c2 and pchi0[bad].min() > 100 * c2
    if loss != RC.NONE:
        assert hev[false, 0].min() > 100 * c2 and hpv[bad, 0].min() > 100 * c2
    dev, dres, ev, pv = L.pose_graph_solve_robust(start, fixed, E, rb, mask=mask, ctx=gpu_ctx, params=p, priors=R, offset=O)
    dpos = max(pose_diff(host[i], dev[i])[0] for i in range(n))
    drot = max(pose_diff(host[i], dev[i])[1] for i in range(n))
    print(f"n {n} {RC.LOSS_NAMES[loss]}: device {dres.iterations} LM / {dres.pcg_iterations} PCG iterations, termination {dres.termination}; host {hres.iterations} / "
          f"{hres.pcg_iterations}, {hres.termination}; {dpos:.2e} m {drot:.2e} rad; cost {dres.initial_cost:.6g} -> {dres.final_cost:.9g} (host {hres.final_cost:.9g})")
    assert dpos <= 1e-7 and drot <= 1e-6
    assert abs(dres.final_cost - hres.final_cost) <= 1e-9 * hres.final_cost
    assert same_bits(dres.initial_cost, hres.initial_cost) or abs(dres.initial_cost - hres.initial_cost) <= 1e-13 * hres.initial_cost
    assert dres.termination in (L.PGO_GRADIENT, L.PGO_STEP) and hres.termination in (L.PGO_GRADIENT, L.PGO_STEP) and dres.message
    assert dres.final_cost < dres.initial_cost and dres.pcg_truncated == 0
    # the verdicts: bit for bit the host's linearization at the poses the device returned
    _, _, chi2, _, w = L.pose_graph_linearize_robust(dev, E, rb, mask=mask)
    _, _, pchi2, _, pw = L.pose_graph_linearize_priors_robust(dev, R, rb, O)
    assert same_bits(ev[:, 0], chi2) and same_bits(ev[:, 1], w) and same_bits(pv[:, 0], pchi2) and same_bits(pv[:, 1], pw)
    assert np.all(ev[~loops, 1] == 1.0)
    if loss != RC.NONE:
        # beyond 100 c2 the weight is below c / sqrt(100 c2) = 0.1 (Huber), far below for the others; a constraint that ends below
        # c2 / 4 as it began keeps at least (1 - 1/4)^2 = 0.5625 (Tukey), 0.64 (Geman-McClure), 1 (Huber)
        # (Huber bounds an outlier's pull, it does not remove it: two fixes of eight 50 m off still move the track by a sigma or
        # two, so only the losses that let go of an outlier are held to the second line)
        assert np.all(ev[false, 1] < 0.1) and np.all(pv[bad, 1] < 0.1)
        if loss != RC.HUBER:
            assert ev[loops & ~false, 0].max() < c2 / 4 and pv[~bad, 0].max() < c2 / 4 and ev[loops & ~false, 1].min() > 0.5625 and pv[~bad, 1].min() > 0.5625
    if loss == RC.TUKEY:
        assert np.all(ev[false, 1] == 0.0) and np.all(pv[bad, 1] == 0.0)
    # twice: identical bits
    again, ares, aev, apv = L.pose_graph_solve_robust(start, fixed, E, rb, mask=mask, ctx=gpu_ctx, params=p, priors=R, offset=O)
    assert same_bits(again, dev) and same_bits(ares.final_cost, dres.final_cost) and same_bits(aev, ev) and same_bits(apv, pv)
    assert (ares.iterations, ares.pcg_iterations, ares.termination) == (dres.iterations, dres.pcg_iterations, dres.termination)


# ---- the Slam calls on the revisit of test_gpu_pose_graph.py: twelve frames forward and back, 23 poses ---------------------------
MODEL, SEED, FORWARD = 16, 1000, 12


@pytest.fixture(scope="module")
def frames(L):
    return [L.synth_frame(MODEL, SEED, f) for f in range(FORWARD + 2)]


def mapped(L, frames, **kw):
    s = L.Slam(0, EgoMotion=3, **{"LoggingTimeout": -1, **kw})
    period = frames[1][1] - frames[0][1]
    order = list(range(FORWARD)) + list(range(FORWARD - 2, -1, -1))
    for f, c in enumerate(order):
        s.add_frame(frames[c][0], frames[0][1] + f * period, f)
    return s, period, len(order)


def Rz(yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    return T


# a registration is trusted to 0.1 m / 0.02 rad here, not to the millimetres its own covariance claims: under that the drift
# of the logged odometry alone is tens of sigmas, and a loss would discount the true loop with the false one
LOOP_INFORMATION = np.diag([1.0 / 0.1**2] * 3 + [1.0 / 0.02**2] * 3)


def loop_edges(L, s):
    """the registered loop, and a false one: the same revisit claimed 30 m away from frame 3"""
    P, t, cov = s.trajectory()
    q = P.shape[0] - 1
    frame, _, _, yaw = s.recognize_place(q, capacity=3, min_travelled=2.0, max_distance=0.0, exclusion_half_window=2)[0]
    reg = s.register_logged_frames(q, frame, L.LoopClosureParams(revisited_half_window=2), P[frame] @ Rz(yaw))
    assert reg.status == 0
    wrong = RC.moved(np.linalg.inv(P[3]) @ P[q], np.array([18.0, -24.0, 0.0]))
    return [(frame, q, reg.relative, LOOP_INFORMATION), (3, q, wrong, LOOP_INFORMATION)]


def snapshot(L, s):
    P, t, cov = s.trajectory()
    return (s.world_transform().tobytes(), s.covariance().tobytes(), [s.map(k).tobytes() for k in (L.EDGE, L.PLANE)], P.tobytes(), t.tobytes())


def two_more(L, s, frames, period, seq):
    shots = []
    for k in range(2):
        s.add_frame(frames[1 + k][0], frames[0][1] + (seq + k) * period, seq + k)
        shots.append(snapshot(L, s))
    return shots


def host_graph(L, P, loops):
    n = len(P)
    W = np.diag(1.0 / np.array(L.PoseGraphParams().odometry_sigma) ** 2)
    chain = [(i - 1, i, np.linalg.inv(P[i - 1]) @ P[i], W) for i in range(1, n)]
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return fixed, chain + list(loops), np.array([0] * (n - 1) + [1] * len(loops), np.uint8)


def test_optimize_trajectory_robust_equals_the_host_statement_and_does_not_touch_the_frame_path(L, frames):
    s, period, n = mapped(L, frames)
    loops = loop_edges(L, s)
    P, t, _ = s.trajectory()
    before = snapshot(L, s)
    fixed, edges, mask = host_graph(L, P, loops)
    for loss in (RC.TUKEY, RC.HUBER, RC.NONE):
        rb = L.PoseGraphRobust(edge_loss=loss, edge_scale=RC.SCALE)
        got, times, res, verdict = L.optimize_trajectory_robust(s, loops, rb)
        assert snapshot(L, s) == before and np.array_equal(times, t) and s.get_param("PoseGraphSeconds") > 0
        host, hres, hev, _ = L.pose_graph_solve_robust(P, fixed, edges, rb, mask=mask)
        d = [pose_diff(host[i], got[i]) for i in range(n)]
        print(f"optimize_trajectory_robust {RC.LOSS_NAMES[loss]}:", res, "against the host statement", max(a for a, _ in d), "m", max(b for _, b in d), "rad; verdicts", verdict)
        assert max(a for a, _ in d) <= 1e-7 and max(b for _, b in d) <= 1e-6
        assert res.termination == hres.termination and res.final_cost <= res.initial_cost
        assert verdict.shape == (2, 2) and np.abs(verdict[:, 1] - hev[-2:, 1]).max() <= 1e-6 and np.abs(verdict[:, 0] - hev[-2:, 0]).max() <= 1e-6 * hev[-2:, 0].max()
        if loss == RC.TUKEY:
            assert verdict[1, 1] == 0.0 and verdict[0, 1] > 0.5  # the false loop is disregarded, the registered one is not
            near = got
        if loss == RC.NONE:
            assert np.all(verdict[:, 1] == 1.0)
            plain_call, _, plain_res = s.optimize_trajectory(loops)  # the existing call is the case of no loss
            assert same_bits(plain_call, got) and same_bits(plain_res.final_cost, res.final_cost)
            clean, _, _ = s.optimize_trajectory(loops[:1])
            far = np.abs(got[:, :3, 3] - clean[:, :3, 3]).max()
            assert far > 0.5 and np.abs(near[:, :3, 3] - clean[:, :3, 3]).max() < far / 10
    # apply=False: two further frames are what they are without the call
    plain, _, _ = mapped(L, frames)
    loop_edges(L, plain)
    assert two_more(L, s, frames, period, n) == two_more(L, plain, frames, period, n)
    plain.close()
    s.close()


def test_optimize_trajectory_robust_applied_equals_set_trajectory(L, frames):
    a, period, n = mapped(L, frames)
    loops = loop_edges(L, a)
    rb = L.PoseGraphRobust(edge_loss=RC.TUKEY, edge_scale=RC.SCALE)
    got, times, res, verdict = L.optimize_trajectory_robust(a, loops, rb, apply=True)
    b, _, _ = mapped(L, frames)
    loop_edges(L, b)
    b.set_trajectory(got, times)
    assert snapshot(L, a) == snapshot(L, b)
    assert two_more(L, a, frames, period, n) == two_more(L, b, frames, period, n)
    # refusals through the common path: nothing changed
    before = snapshot(L, a)
    for bad in ([(0, 99, np.eye(4), np.eye(6))], [(-1, 3, np.eye(4), np.eye(6))], [(3, 3, np.eye(4), np.eye(6))]):
        with pytest.raises(L.LsaError) as e:
            L.optimize_trajectory_robust(a, bad, rb, apply=True)
        assert e.value.code == L.E_ARG
    for bad in (L.PoseGraphRobust(edge_loss=5), L.PoseGraphRobust(edge_loss=RC.HUBER, edge_scale=0.0)):
        with pytest.raises(L.LsaError) as e:
            L.optimize_trajectory_robust(a, loops, bad, apply=True)
        assert e.value.code == L.E_ARG
    with pytest.raises(L.LsaError) as e:
        L.optimize_trajectory_robust(a, loops, rb, odometry_sigma=[0.0] * 6)
    assert e.value.code == L.E_ARG
    assert snapshot(L, a) == before
    off = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    for f in range(3):
        off.add_frame(frames[f][0], frames[f][1], f)
    with pytest.raises(L.LsaError) as e:
        L.optimize_trajectory_robust(off, [], rb)
    assert e.value.code == L.E_STATE and "LoggingTimeout" in str(e.value)
    off.close()
    a.close()
    b.close()


def test_run_pose_graph_optimization_robust_against_the_host_statement(L, frames):
    """Fixes of 0.5 m bent by up to 0.2 m, fix 7 50 m off, and one more fix five seconds after the log, which matches no pose.
    Huber: the start is the track laid onto ALL the fixes, the outlying one included, which puts every fix metres off at first --
    under a loss that is flat beyond its scale (Tukey) nothing would pull from there; the convex loss has one minimum."""
    s, period, n = mapped(L, frames)
    P, t, lcov = s.trajectory()
    Wt, O = PP.world_transform(), PP.lever_arm()
    g = np.array([(Wt @ P[i] @ O)[:3, 3] for i in range(n)]) + 0.2 * np.sin(np.pi * np.arange(n) / (n - 1))[:, None] * np.array([0.0, 0.8, 0.6])
    g[7] += np.array([0.0, 30.0, 40.0])
    gt, gx = np.concatenate([t, [t[-1] + 5.0]]), np.concatenate([g, g[-1:]])
    cov = np.repeat((np.eye(3) * 0.5**2)[None], n + 1, 0)
    before = snapshot(L, s)
    rb = L.PoseGraphRobust(prior_loss=RC.HUBER, prior_scale=RC.SCALE, edge_loss=RC.TUKEY, edge_scale=1e-3)  # edge_loss has no say here: the chain is never discounted
    got, times, cal, res, matches, verdict = L.run_pose_graph_optimization_robust(s, gt, gx, cov, rb, gps_to_sensor=np.linalg.inv(O), apply=False)
    assert snapshot(L, s) == before and list(matches) == list(range(n)) + [-1]
    lcov = np.asarray(lcov).reshape(n, 6, 6)
    chain = [(i - 1, i, np.linalg.inv(P[i - 1]) @ P[i], L.information_from_covariance(lcov[i])) for i in range(1, n)]
    priors = [(i, g[i], L.information_from_covariance3(cov[i])) for i in range(n)]
    W = L.trajectory_alignment([(P[i] @ O)[:3, 3] for i in range(n)], g)
    start = L.pose_graph_premultiply(P, W)
    hrb = L.PoseGraphRobust(prior_loss=RC.HUBER, prior_scale=RC.SCALE)
    host, hres, hev, hpv = L.pose_graph_solve_robust(start, np.zeros(n, np.uint8), chain, hrb, priors=priors, offset=O, odometry_information=1)
    back = L.pose_graph_reanchor(host)
    d = [pose_diff(back[i], got[i]) for i in range(n)]
    print("outlying fix:", res, "against the host statement", max(x for x, _ in d), "m", max(y for _, y in d), "rad; verdicts", verdict[[0, 7, n]])
    assert max(x for x, _ in d) <= 1e-7 and max(y for _, y in d) <= 1e-6
    assert res.termination == hres.termination and res.final_cost < res.initial_cost
    assert verdict.shape == (n + 1, 2) and verdict[n, 1] == -1.0 and verdict[n, 0] == 0.0  # the unmatched fix
    assert verdict[7, 1] < 0.05 and verdict[7, 0] > 100 * RC.SCALE**2
    assert np.abs(verdict[:n, 1] - hpv[:, 1]).max() <= 1e-6 and np.delete(verdict[:n, 1], 7).min() > 0.9
    # without the loss the fix drags the track; with it the track is the one of the inlying fixes
    none, _, _, _, _ = s.run_pose_graph_optimization(gt, gx, cov, gps_to_sensor=np.linalg.inv(O), apply=False)
    keep = np.arange(n + 1) != 7
    clean, _, _, _, _ = s.run_pose_graph_optimization(gt[keep], gx[keep], cov[keep], gps_to_sensor=np.linalg.inv(O), apply=False)
    far = np.abs(none[:, :3, 3] - clean[:, :3, 3]).max()
    assert far > 0.5 and np.abs(got[:, :3, 3] - clean[:, :3, 3]).max() < far / 10
    # no loss: the existing call's bits, every matched fix weighs 1
    same, _, _, _, _, v1 = L.run_pose_graph_optimization_robust(s, gt, gx, cov, L.PoseGraphRobust(), gps_to_sensor=np.linalg.inv(O), apply=False)
    assert same_bits(same, none) and np.all(v1[:n, 1] == 1.0) and v1[n, 1] == -1.0
    with pytest.raises(L.LsaError) as e:
        L.run_pose_graph_optimization_robust(s, gt, gx, cov, L.PoseGraphRobust(prior_loss=9), gps_to_sensor=np.linalg.inv(O))
    assert e.value.code == L.E_ARG and snapshot(L, s) == before
    s.close()


# ---- the example ------------------------------------------------------------------------------------------------------------------
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_robust_pose_graph")
    forward = 12
    r = subprocess.run([exe, "16", str(forward)], capture_output=True, text=True, check=True)
    extra = {}
    for line in r.stdout.strip().splitlines():
        if line.startswith("#"):
            words = line.split()[1:]
            extra.setdefault(words[0], []).append([float(v) for v in words[1:]])
    frames = [L.synth_frame(16, 1000, f) for f in range(forward)]
    s, period, n = mapped(L, frames)
    loops = loop_edges(L, s)
    assert extra["edge"] == [[loops[0][0], loops[0][1]], [loops[1][0], loops[1][1]]]
    none, _, res0, v0 = L.optimize_trajectory_robust(s, loops, L.PoseGraphRobust())
    got, _, res, v = L.optimize_trajectory_robust(s, loops, L.PoseGraphRobust(edge_loss=RC.TUKEY, edge_scale=3.0), apply=True)
    assert extra["solve"] == [[0, res0.termination, res0.iterations, res0.pcg_iterations], [3, res.termination, res.iterations, res.pcg_iterations]]
    assert np.allclose(extra["cost"], [[res0.initial_cost, res0.final_cost], [res.initial_cost, res.final_cost]], rtol=1e-8, atol=0)
    assert np.allclose(extra["verdict"], [[0, 0, v0[0, 0], 1.0], [0, 1, v0[1, 0], 1.0], [3, 0, v[0, 0], v[0, 1]], [3, 1, v[1, 0], v[1, 1]]], rtol=1e-7, atol=1e-12)
    assert extra["verdict"][3][3] == 0.0
    assert np.allclose(extra["last"], [none[-1][:3, 3], got[-1][:3, 3]], atol=1e-9, rtol=0)
    for k in range(2):
        s.add_frame(frames[1 + k][0], frames[0][1] + (n + k) * period, n + k)
        assert np.allclose(extra["frame"][k], s.world_transform()[:3, 3], atol=1e-9, rtol=0)
    s.close()
