"""Robust losses in the pose graph, the host statement (lidarslam_amd/csrc/host/lsa_pose_graph.cpp over the section ROBUST LOSS of
lsa_pose_graph.h): the loss function against mpmath, the weighted linearization bit for bit, the solve against an independent
dense numpy IRLS-LM (tests/pose_graph_robust_cases.py), the verdicts, and what the feature is for.  No GPU."""
import ctypes as C
import functools
import os
import platform
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest

import pose_graph_cases as PG
import pose_graph_prior_cases as PP
import pose_graph_robust_cases as RC
from conftest import pose_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = PG.EPS
SCALES = [0.5, 1.0, 3.0]


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def loss_points(c):
    c2 = c * c  # exact: 0.25, 1, 9
    return [0.0, 1e-300, 1e-12 * c2, c2 * (1.0 - 2.0**-52), c2, float(np.nextafter(c2, np.inf)), 4.0 * c2, 1e12 * c2]


def exact_loss(loss, c, s):
    """-> rho(s) as an mpmath function of the branch s lies in, and the bounds (rho, w) of the double evaluation.

    Each bound is n eps (sum of the magnitudes of the formula's terms), n the number of roundings of the formula as
    lsa_pose_graph.h writes it (c, 2 c, c2 = c c and 3 are exact here); eps = 2^-52 is twice the unit roundoff, which pays for a
    rounded value entering a product twice (q q, v v).
      NONE, Huber and Tukey where they are s, 1, 0: exact, bound 0.
      Huber, s > c2: r = sqrt(s) [1]; (2 c) r [2]; - c2 [3]: 3 eps (2 c r + c2).  w = c / r: [2], 2 eps (c / r).
      Geman-McClure: d = c2 + s [1]; c2 s [2]; the quotient [3]: one product chain, 3 eps rho.  q = c2 / d [2]; q q [3]: 3 eps w.
      Tukey, s > c2: c2 / 3 [1]: eps c2 / 3.
      Tukey, else: t = s / c2 [1]; v = 1 - t [2]; 1 + v [3]; v v [4]; their sum [5]; s / 3 [6]; the product [7]: 7 eps (s / 3)
        (1 + |v| + v^2).  w = v v with v = 1 - t: t [1], v [2], v v [3] -- v is a difference, so the terms are those of the
        expanded square 1 - 2 t + t^2: 3 eps (1 + t)^2 (next to s = c2, where v cancels to nothing, this is all that can be said)."""
    c, s = mp.mpf(c), mp.mpf(s)
    c2 = c * c
    if loss == RC.HUBER and s > c2:
        r = mp.sqrt(s)
        return (lambda x: 2 * c * mp.sqrt(x) - c2), 3 * EPS * float(2 * c * r + c2), 2 * EPS * float(c / r)
    if loss == RC.GEMAN_MCCLURE:
        f = lambda x: c2 * x / (c2 + x)  # noqa: E731
        return f, 3 * EPS * float(f(s)), 3 * EPS * float((c2 / (c2 + s)) ** 2)
    if loss == RC.TUKEY:
        if s > c2:
            return (lambda x: c2 / 3 + 0 * x), EPS * float(c2 / 3), 0.0
        t = s / c2
        v = 1 - t
        # c2/3 (1 - (1 - x/c2)^3) multiplied out: at x = 1e-300 the cube would need 300 digits
        return (lambda x: x - x * x / c2 + x * x * x / (3 * c2 * c2)), 7 * EPS * float(s / 3 * (1 + abs(v) + v * v)), 3 * EPS * float((1 + t) ** 2)
    return (lambda x: x), 0.0, 0.0


@pytest.mark.parametrize("c", SCALES)
@pytest.mark.parametrize("loss", RC.LOSSES)
def test_rho_and_w_against_mpmath(L, loss, c):
    mp.mp.dps = 50
    worst = [0.0, 0.0]
    got = {}
    for s in loss_points(c):
        rho, w = L.pose_graph_robust_rho(loss, c, s)
        f, brho, bw = exact_loss(loss, c, s)
        rho_ref = f(mp.mpf(s))
        with mp.workdps(150):  # the derivative by differences: a weight of 1e-24 next to a cost of 9 needs the digits
            w_ref = mp.diff(f, mp.mpf(s))
        erho, ew = abs(float(mp.mpf(rho) - rho_ref)), abs(float(mp.mpf(w) - w_ref))
        assert erho <= brho, (RC.LOSS_NAMES[loss], c, s, rho, float(rho_ref), erho, brho)
        assert ew <= bw, (RC.LOSS_NAMES[loss], c, s, w, float(w_ref), ew, bw)
        # the closed form of the weight too
        cw = RC.rho_w(loss, c, s)[1]
        assert abs(w - cw) <= bw + 4 * EPS * abs(cw)
        worst = [max(worst[0], erho / brho if brho else 0.0), max(worst[1], ew / bw if bw else 0.0)]
        got[s] = (rho, w, brho, bw)
    # continuity across s = c2: rho' = w <= 1 and |w'| <= 2 / c2 everywhere, so two points ds apart differ by no more than that
    pts = loss_points(c)[3:6]
    for a, b in ((pts[0], pts[1]), (pts[1], pts[2])):
        ds = b - a
        assert abs(got[a][0] - got[b][0]) <= got[a][2] + got[b][2] + ds
        assert abs(got[a][1] - got[b][1]) <= got[a][3] + got[b][3] + 2.0 * ds / (c * c)
    print(f"{RC.LOSS_NAMES[loss]} c {c}: worst error / bound  rho {worst[0]:.3f}  w {worst[1]:.3f}")


def test_the_loss_at_zero_and_a_nan(L):
    for loss in RC.LOSSES:
        assert L.pose_graph_robust_rho(loss, 2.0, 0.0) == (0.0, 1.0)
        rho, w = L.pose_graph_robust_rho(loss, 2.0, float("nan"))
        assert np.isnan(rho)  # the outer branch is taken only when s > c2 is true: a NaN chi2 stays a NaN cost
    rho, w = L.pose_graph_robust_rho(np.int32(RC.TUKEY), 2.0, np.array([[1.0, 5.0]]))
    assert rho.shape == (1, 2) and w[0, 1] == 0.0


def test_robust_struct_is_the_headers(L):
    r = L.PoseGraphRobust()
    assert (r.edge_loss, r.prior_loss, r.edge_scale, r.prior_scale) == (L.PGO_LOSS_NONE, L.PGO_LOSS_NONE, 1.0, 1.0)
    assert C.sizeof(L.PoseGraphRobust) == 24 and [getattr(L.PoseGraphRobust, f).offset for f, _ in L.PoseGraphRobust._fields_] == [0, 4, 8, 16]
    assert (L.PGO_LOSS_NONE, L.PGO_LOSS_HUBER, L.PGO_LOSS_GEMAN_MCCLURE, L.PGO_LOSS_TUKEY) == (0, 1, 2, 3)
    with pytest.raises(TypeError):
        L.PoseGraphRobust(loss=1)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
BAD_ROBUST = [dict(edge_loss=4), dict(edge_loss=-1), dict(prior_loss=7), dict(edge_loss=1, edge_scale=0.0), dict(edge_loss=2, edge_scale=-1.0),
              dict(edge_loss=3, edge_scale=float("nan")), dict(prior_loss=1, prior_scale=float("inf")), dict(prior_loss=3, prior_scale=0.0)]


def raw_solve(L, poses, fixed, edges, priors, O, robust, mask=None):
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    E, R = L.pose_graph_edges(edges), L.pose_graph_priors(priors)
    Om = np.ascontiguousarray(np.asarray(O, np.float64).reshape(16))
    f = np.ascontiguousarray(fixed, np.uint8)
    out, ev, pv = np.full_like(P, -7.0), np.full((E.size, 2), -7.0), np.full((max(R.size, 1), 2), -7.0)
    r = L.PoseGraphResultStruct()
    r.iterations = -7
    p = L.PoseGraphParams()
    rc = L.lib().lsa_pgo_solve_robust_host(L.ptr(P), P.shape[0], L.ptr(f), L.ptr(E), E.size, None if mask is None else L.ptr(mask), L.ptr(R) if R.size else None, R.size,
                                           L.ptr(Om), C.byref(p), None if robust is None else C.byref(robust), L.ptr(out), C.byref(r), L.ptr(ev), L.ptr(pv))
    return rc, out, r, ev, pv


def test_refusals_leave_the_outputs_untouched(L):
    start, fixed, edges, mask, priors, O, _, _ = RC.robust_gps_graph(16, 3, (1,))
    E, R = L.pose_graph_edges(edges), L.pose_graph_priors(priors)
    P = np.ascontiguousarray(start.reshape(-1, 16))
    Om = np.ascontiguousarray(O.reshape(16))
    for bad in BAD_ROBUST:
        rb = L.PoseGraphRobust(**bad)
        rc, out, r, ev, pv = raw_solve(L, start, fixed, edges, priors, O, rb, mask)
        assert rc == L.E_ARG and np.all(out == -7.0) and r.iterations == -7 and np.all(ev == -7.0) and np.all(pv == -7.0), bad
        outs = [np.full((E.size, 6), -7.0), np.full((E.size, 120), -7.0)] + [np.full(E.size, -7.0) for _ in range(3)]
        assert L.lib().lsa_pgo_linearize_robust_host(L.ptr(P), P.shape[0], L.ptr(E), E.size, L.ptr(mask), C.byref(rb), *[L.ptr(o) for o in outs]) == L.E_ARG
        assert all(np.all(o == -7.0) for o in outs)
        outs = [np.full((R.size, 3), -7.0), np.full((R.size, 42), -7.0)] + [np.full(R.size, -7.0) for _ in range(3)]
        assert L.lib().lsa_pgo_linearize_robust_priors_host(L.ptr(P), P.shape[0], L.ptr(R), R.size, L.ptr(Om), C.byref(rb), *[L.ptr(o) for o in outs]) == L.E_ARG
        assert all(np.all(o == -7.0) for o in outs)
        with pytest.raises(L.LsaError):
            L.pose_graph_solve_robust(start, fixed, edges, rb, mask=mask, priors=priors, offset=O)
    for loss, scale in ((4, 1.0), (-1, 1.0), (1, 0.0), (2, -2.0), (3, float("nan")), (1, float("inf"))):
        a, b = C.c_double(-7.0), C.c_double(-7.0)
        assert L.lib().lsa_pgo_robust_rho_host(loss, scale, 1.0, C.byref(a), C.byref(b)) == L.E_ARG and a.value == b.value == -7.0
        with pytest.raises(L.LsaError):
            L.pose_graph_robust_rho(loss, scale, 1.0)
    # a scale is not looked at while its loss is NONE
    rc, out, _, _, _ = raw_solve(L, start, fixed, edges, priors, O, L.PoseGraphRobust(edge_scale=-1.0, prior_scale=float("nan")), mask)
    assert rc == 0 and np.isfinite(out).all()
    # a mask of another length than the edges; something that is no PoseGraphRobust
    rb = L.PoseGraphRobust(edge_loss=L.PGO_LOSS_TUKEY, edge_scale=3.0)
    for wrong in (mask[:-1], np.concatenate([mask, [1]]), np.zeros(0, np.uint8)):
        for call in (lambda: L.pose_graph_solve_robust(start, fixed, edges, rb, mask=wrong, priors=priors, offset=O), lambda: L.pose_graph_linearize_robust(start, edges, rb, mask=wrong)):
            with pytest.raises(L.LsaError) as info:
                call()
            assert info.value.code == L.E_ARG
    with pytest.raises(L.LsaError):
        L.pose_graph_solve_robust(start, fixed, edges, None, priors=priors, offset=O)
    # the graph's own refusals go on holding
    rc, out, r, ev, pv = raw_solve(L, start, fixed, edges, [], O, rb, mask)  # no fixed pose and no prior
    assert rc == L.E_ARG and np.all(out == -7.0) and np.all(ev == -7.0)


# ---- NONE is the solver as it was ---------------------------------------------------------------------------------------------
def result_fields(r):
    return [(name, getattr(r, name)) for name, _ in r._fields_]


@pytest.mark.parametrize("graph", ["features", "circle64", "gps16", "gps64"])
def test_no_loss_gives_the_bits_of_the_solve_without_losses(L, graph):
    if graph == "features":
        (poses, fixed, edges), (priors, O) = PG.feature_graph(), PP.feature_priors()
    elif graph == "circle64":
        (poses, fixed, edges), priors, O = PG.circle_graph(64)[:3], [], np.eye(4)
    else:
        _, poses, fixed, edges, priors, O, _ = PP.gps_case(int(graph[3:]), 3)
    for with_priors in ([False, True] if len(priors) and fixed.any() else [bool(len(priors))]):
        pr = priors if with_priors else None
        ref, rref = L.pose_graph_solve_host(poses, fixed, edges, priors=pr, offset=O)
        assert rref.iterations > 0
        m = len(edges)
        alternating = (np.arange(m) % 2).astype(np.uint8)
        for rb, mask in ((L.PoseGraphRobust(), None), (L.PoseGraphRobust(), alternating), (L.PoseGraphRobust(edge_scale=0.5, prior_scale=7.0), None)) + tuple(
                (L.PoseGraphRobust(edge_loss=loss, edge_scale=1.0), np.zeros(m, np.uint8)) for loss in RC.LOSSES[1:]):
            out, r, ev, pv = L.pose_graph_solve_robust(poses, fixed, edges, rb, mask=mask, priors=pr, offset=O)
            assert same_bits(out, ref), (graph, rb.edge_loss)
            for name in ("initial_cost", "final_cost", "largest_step", "final_lambda"):
                assert same_bits(getattr(r, name), getattr(rref, name)), name
            assert (r.iterations, r.accepted_steps, r.rejected_steps, r.pcg_iterations, r.termination) == (
                rref.iterations, rref.accepted_steps, rref.rejected_steps, rref.pcg_iterations, rref.termination)
            # the verdicts of constraints that are not robustified: chi2 at the returned poses, weight 1
            assert same_bits(ev[:, 0], L.pose_graph_linearize(out, edges)[2]) and np.all(ev[:, 1] == 1.0)
            if with_priors:
                assert same_bits(pv[:, 0], L.pose_graph_linearize_priors(out, priors, O)[2]) and np.all(pv[:, 1] == 1.0)
    # the raw entry with robust = NULL is init
    rc0, out0, r0, _, _ = raw_solve(L, poses, fixed, edges, priors, O, None)
    rc1, out1, r1, _, _ = raw_solve(L, poses, fixed, edges, priors, O, L.PoseGraphRobust())
    assert rc0 == rc1 == 0 and same_bits(out0, out1) and result_fields(r0)[:-1] == result_fields(r1)[:-1]


# ---- the linearization is the product with the weight ---------------------------------------------------------------------------
@pytest.mark.parametrize("loss", RC.LOSSES)
def test_robust_linearization_is_the_weight_times_the_plain_one(L, loss):
    """Masked and unmasked edges interleaved, scales that put edges on both sides of c2; bit for bit: the definition is that product."""
    poses, _, edges = PG.feature_graph()
    priors, O = PP.feature_priors()
    e0, b0, c0 = L.pose_graph_linearize(poses, edges)
    mask = (np.arange(len(edges)) % 2 == 0).astype(np.uint8)
    c = float(np.sqrt(np.median(c0)))
    rb = L.PoseGraphRobust(edge_loss=loss, edge_scale=c, prior_loss=loss, prior_scale=2.0)
    for mk in (mask, None, np.zeros_like(mask)):
        e, b, chi2, rho, w = L.pose_graph_linearize_robust(poses, edges, rb, mask=mk)
        sel = np.ones(len(edges), bool) if mk is None else mk.astype(bool)
        rho_ref, w_ref = L.pose_graph_robust_rho(loss, c, c0)
        rho_ref, w_ref = np.where(sel, rho_ref, c0), np.where(sel, w_ref, 1.0)
        assert same_bits(e, e0) and same_bits(chi2, c0) and same_bits(rho, rho_ref) and same_bits(w, w_ref)
        assert same_bits(b, w_ref[:, None] * b0)
        if loss in (RC.HUBER, RC.TUKEY) and mk is not None and mk.any():
            assert (c0[sel] > c * c).any() and (c0[sel] <= c * c).any()  # both branches
        if loss != RC.NONE and sel.any():
            assert (w[sel] < 1.0).any() and np.all(w[~sel] == 1.0)
    pe0, pb0, pc0 = L.pose_graph_linearize_priors(poses, priors, O)
    pe, pb, pchi2, prho, pw = L.pose_graph_linearize_priors_robust(poses, priors, rb, O)
    rho_ref, w_ref = L.pose_graph_robust_rho(loss, 2.0, pc0)
    assert same_bits(pe, pe0) and same_bits(pchi2, pc0) and same_bits(prho, rho_ref) and same_bits(pw, w_ref) and same_bits(pb, w_ref[:, None] * pb0)
    # against the numpy statement too (sums of a few products, as tests/test_pose_graph_host.py holds the plain blocks)
    _, b_np, c_np = RC.linearize(poses, edges)
    e, b, chi2, rho, w = L.pose_graph_linearize_robust(poses, edges, rb, mask=mask)
    w_np = np.array([RC.rho_w(loss if mask[k] else RC.NONE, c, s)[1] for k, s in enumerate(c_np)])
    assert np.abs(b - w_np[:, None] * b_np).max() <= 1e-11 * np.abs(b_np).max()


# ---- the solve against the dense numpy IRLS-LM ------------------------------------------------------------------------------------
CASES = ["loops16", "loops64", "loops200", "gps64"]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> start, fixed, edges, mask, is_false (m,), priors, O, is_outlier (k,)"""
    if name.startswith("loops"):
        init, fixed, edges, mask, false, _ = RC.robust_graph(int(name[5:]))
        return init, fixed, edges, mask, false, [], np.eye(4), np.zeros(0, bool)
    start, fixed, edges, mask, priors, O, bad, _ = RC.robust_gps_graph(int(name[3:]), 4)
    return start, fixed, edges, mask, np.zeros(len(edges), bool), priors, O, bad


@functools.lru_cache(maxsize=None)
def numpy_solve(name, loss):
    """the dense numpy IRLS-LM on a case, once: -> poses, F, F0, termination, verdicts at the start and at the end"""
    start, fixed, edges, mask, false, priors, O, bad = case(name)
    rb = RC.Robust(loss, RC.SCALE, loss, RC.SCALE, mask)
    import lidarslam_amd

    ref, F, F0, term, its = RC.dense_lm(start, fixed, edges, priors, O, lidarslam_amd.PoseGraphParams(), rb)
    return ref, F, F0, term, RC.verdicts(start, edges, priors, O, rb), RC.verdicts(ref, edges, priors, O, rb)


def check_input_conditions(name, loss):
    """The outcome must not hang on the path: every false constraint starts and ends with chi2 > 100 c2 (it is in the flat or
    the linear part of its loss all the way), every true loop starts with chi2 < c2 / 4.  On the numpy side.  Without a loss
    there is no scale and no branch, and the false edges bend the track: the start alone is looked at."""
    start, fixed, edges, mask, false, priors, O, bad = case(name)
    (ev0, pv0), (ev1, pv1) = numpy_solve(name, loss)[4:]
    c2 = RC.SCALE**2
    true_loops = mask.astype(bool) & ~false
    assert true_loops.any() and ev0[true_loops, 0].max() < c2 / 4
    for v0, v1, sel in ((ev0, ev1, false), (pv0, pv1, bad)):
        if sel.any():
            assert v0[sel, 0].min() > 100 * c2 and (loss == RC.NONE or v1[sel, 0].min() > 100 * c2)
    if len(priors):
        assert pv0[~bad, 0].max() < c2 / 4


@pytest.mark.parametrize("loss", RC.LOSSES)
@pytest.mark.parametrize("name", CASES)
def test_solve_against_a_dense_numpy_irls_lm(L, name, loss):
    """1e-8 m / 1e-7 rad and 1e-9 of the cost: the project's tolerances for the host statement against numpy."""
    start, fixed, edges, mask, false, priors, O, bad = case(name)
    n = len(start)
    check_input_conditions(name, loss)
    ref, F_ref, F0_ref, term_ref, _, (ev_ref, pv_ref) = numpy_solve(name, loss)
    rb = L.PoseGraphRobust(edge_loss=loss, edge_scale=RC.SCALE, prior_loss=loss, prior_scale=RC.SCALE)
    out, res, ev, pv = L.pose_graph_solve_robust(start, fixed, edges, rb, mask=mask, priors=priors if len(priors) else None, offset=O)
    dpos = max(pose_diff(ref[i], out[i])[0] for i in range(n))
    drot = max(pose_diff(ref[i], out[i])[1] for i in range(n))
    print(f"{name} {RC.LOSS_NAMES[loss]}: {res.iterations} LM iterations, {res.pcg_iterations} PCG iterations, termination {res.termination} (numpy {term_ref}); against numpy "
          f"{dpos:.2e} m {drot:.2e} rad, cost {res.initial_cost:.6g} -> {res.final_cost:.6g} (rel {abs(res.final_cost - F_ref) / F_ref:.1e})")
    assert res.termination in (L.PGO_GRADIENT, L.PGO_STEP, L.PGO_COST) and term_ref in (1, 2, 3)
    assert abs(res.initial_cost - F0_ref) <= 1e-12 * F0_ref
    assert dpos <= 1e-8 and drot <= 1e-7
    assert abs(res.final_cost - F_ref) <= 1e-9 * F_ref
    assert res.final_cost < res.initial_cost and res.accepted_steps >= 1 and res.pcg_truncated == 0
    # the verdicts: chi2 and the weight of every constraint at the returned poses
    assert ev.shape == ev_ref.shape and pv.shape == pv_ref.shape
    for got, want in ((ev, ev_ref), (pv, pv_ref)):
        if got.size:
            assert np.abs(got[:, 0] - want[:, 0]).max() <= 1e-6 * np.maximum(1.0, want[:, 0]).max()
            assert np.abs(got[:, 1] - want[:, 1]).max() <= 1e-6
    assert np.all(ev[mask == 0, 1] == 1.0)  # the odometry chain is not robustified
    # and bit for bit what the linearization says at those poses
    _, _, chi2, _, w = L.pose_graph_linearize_robust(out, edges, rb, mask=mask)
    assert same_bits(ev[:, 0], chi2) and same_bits(ev[:, 1], w)
    if len(priors):
        _, _, pchi2, _, pw = L.pose_graph_linearize_priors_robust(out, priors, rb, O)
        assert same_bits(pv[:, 0], pchi2) and same_bits(pv[:, 1], pw)


# ---- what the feature is for ------------------------------------------------------------------------------------------------------
def test_false_loops_are_disregarded(L):
    """N = 200, three true and two false loops.  `clean`: the plain solve of the graph without the false edges.  Under every loss the
    track stays ten times nearer to it than the plain solve of the whole graph does; under Tukey every false edge's verdict
    weight is exactly 0 and every true loop's is above 0.9.  First the numpy statement alone shows that the inputs give these
    margins; then the library is held to them."""
    init, fixed, edges, mask, false, _ = RC.robust_graph(200)
    ci, cf, ce, _, _, _ = RC.robust_graph(200, False)
    assert np.array_equal(ci, init) and len(ce) == len(edges) - int(false.sum())
    p = L.PoseGraphParams()
    clean_np = RC.dense_lm(ci, cf, ce, [], None, p, RC.Robust())[0]
    far_np = np.abs(numpy_solve("loops200", RC.NONE)[0][:, :3, 3] - clean_np[:, :3, 3]).max()
    assert far_np > 0.5  # the false edges bend the track by more than half a metre
    loops = mask.astype(bool)
    for loss in RC.LOSSES[1:]:
        ref, _, _, _, _, (ev_np, _) = numpy_solve("loops200", loss)
        assert np.abs(ref[:, :3, 3] - clean_np[:, :3, 3]).max() < far_np / 20  # twice the margin asked of the library
        if loss == RC.TUKEY:
            assert np.all(ev_np[false, 1] == 0.0) and ev_np[loops & ~false, 1].min() > 0.95
    clean, _ = L.pose_graph_solve_host(ci, cf, ce)
    none, _, ev, _ = L.pose_graph_solve_robust(init, fixed, edges, L.PoseGraphRobust(), mask=mask)
    far = np.abs(none[:, :3, 3] - clean[:, :3, 3]).max()
    assert np.all(ev[:, 1] == 1.0) and ev[false, 0].min() > 1e3
    for loss in RC.LOSSES[1:]:
        out, res, ev, _ = L.pose_graph_solve_robust(init, fixed, edges, L.PoseGraphRobust(edge_loss=loss, edge_scale=RC.SCALE), mask=mask)
        near = np.abs(out[:, :3, 3] - clean[:, :3, 3]).max()
        print(f"{RC.LOSS_NAMES[loss]}: {near:.4f} m from the clean solve (no loss: {far:.4f} m); weights of the loops {np.round(ev[loops, 1], 4)}")
        assert near < far / 10
        assert np.all(ev[false, 1] < 0.05) and np.all(ev[~loops, 1] == 1.0)
        if loss == RC.TUKEY:
            assert np.all(ev[false, 1] == 0.0) and ev[loops & ~false, 1].min() > 0.9


def test_an_outlying_fix_is_disregarded(L):
    start, fixed, edges, mask, priors, O, bad, _ = RC.robust_gps_graph(64, 4)
    inliers = [pr for pr, b in zip(priors, bad) if not b]
    clean, _ = L.pose_graph_solve_host(start, fixed, edges, priors=inliers, offset=O)
    none, _ = L.pose_graph_solve_host(start, fixed, edges, priors=priors, offset=O)
    far = np.abs(none[:, :3, 3] - clean[:, :3, 3]).max()
    out, _, ev, pv = L.pose_graph_solve_robust(start, fixed, edges, L.PoseGraphRobust(prior_loss=L.PGO_LOSS_TUKEY, prior_scale=RC.SCALE), priors=priors, offset=O)
    assert far > 0.5 and np.abs(out[:, :3, 3] - clean[:, :3, 3]).max() < far / 10
    assert np.all(pv[bad, 1] == 0.0) and pv[~bad, 1].min() > 0.9 and np.all(ev[:, 1] == 1.0)


# ---- the host statement under the sanitizers ---------------------------------------------------------------------------------------
def test_host_statement_with_losses_under_the_sanitizers(tmp_path):
    """tests/pose_graph_robust_sanitize.cpp: the loss function at the values above, the weighted linearization and a robust solve
    with its verdicts, with their own main under -fsanitize=address,undefined, built and run as tests/pose_graph_sanitize.cpp is"""
    host = os.path.join(ROOT, "lidarslam_amd", "csrc", "host")
    exe = str(tmp_path / "pose_graph_robust_sanitize")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags + ["-I" + host, os.path.join(ROOT, "tests", "pose_graph_robust_sanitize.cpp"),
                                                                             os.path.join(host, "lsa_pose_graph.cpp"), "-o", exe]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler has no runtime for -fsanitize=address,undefined")
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    norand = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") is None or subprocess.run(norand + ["true"], capture_output=True).returncode != 0:
        norand = []
    run = subprocess.run(norand + [exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr


def test_the_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path, L):
    """examples/slam_robust_pose_graph.cpp through the C++ mirror; with a GPU tests/test_gpu_pose_graph_robust.py runs it"""
    from test_cpp_api import build_example

    exe = build_example(tmp_path, "slam_robust_pose_graph")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr
