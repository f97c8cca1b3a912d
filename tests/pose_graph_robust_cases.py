"""Robust losses in the pose graph: the independent numpy statement and the graphs the tests share
(tests/test_pose_graph_robust_host.py, test_gpu_pose_graph_robust.py).  Extends tests/pose_graph_cases.py and
tests/pose_graph_prior_cases.py, whose edge and prior statements it uses; written from the table ROBUST LOSS of
lidarslam_amd/csrc/lsa_pose_graph.h's comment in its closed forms, it shares no code with the C++.

A loss acts on s = chi2 of one constraint at scale c: rho(s) enters the cost F = 1/2 sum rho, w = rho'(s) multiplies the
constraint's block record (first-order IRLS).
"""
import functools

import numpy as np

import pose_graph_cases as PG
import pose_graph_prior_cases as PP

NONE, HUBER, GEMAN_MCCLURE, TUKEY = range(4)
LOSSES = [NONE, HUBER, GEMAN_MCCLURE, TUKEY]
LOSS_NAMES = ["none", "huber", "geman-mcclure", "tukey"]


def rho_w(loss, c, s):
    """(rho, w) in the closed forms: Huber 2 c sqrt(s) - c^2, Geman-McClure c^2 s / (c^2 + s), Tukey c^2/3 (1 - (1 - s/c^2)^3)"""
    c2 = c * c
    if loss == HUBER and s > c2:
        return 2.0 * c * np.sqrt(s) - c2, c / np.sqrt(s)
    if loss == GEMAN_MCCLURE:
        return c2 * s / (c2 + s), (c2 / (c2 + s)) ** 2
    if loss == TUKEY:
        if s > c2:
            return c2 / 3.0, 0.0
        return c2 / 3.0 * (1.0 - (1.0 - s / c2) ** 3), (1.0 - s / c2) ** 2
    return s, 1.0


def log_so3(R):
    """PG.log_so3 with one more case: for an angle below a right angle, v (theta / sin theta) at every size of the angle.
    PG.log_so3 takes angles between 1e-7 and 1e-4 rad through the eigenvector of R's symmetric part, whose eigenvalues 1 and
    cos(theta) lie theta^2 / 2 apart there: the axis is good to eps / theta^2 and the cost of an edge weighted 1 / (0.2 mrad)^2
    to 1e-8 only, which is the size of the last LM steps' decrease in these graphs (residual rotations of 1e-5 rad)."""
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = float(np.linalg.norm(v)), 0.5 * (np.trace(R) - 1.0)
    if c > 0 and s >= 1e-7:
        return v * (float(np.arctan2(s, c)) / s)
    return PG.log_so3(R)


def edge_jacobians(Ti, Tj, Z):
    """PG.edge_jacobians over the log above"""
    Ri, Rj, Rz = Ti[:3, :3], Tj[:3, :3], Z[:3, :3]
    d = Ri.T @ (Tj[:3, 3] - Ti[:3, 3])
    Rij = Ri.T @ Rj
    RE = Rz.T @ Rij
    e = np.concatenate([Rz.T @ (d - Z[:3, 3]), log_so3(RE)])
    J = PG.jr_inv(e[3:])
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    A[:3, :3], A[:3, 3:], A[3:, 3:] = -Rz.T, Rz.T @ PG.hat(d), -J @ Rij.T
    B[:3, :3], B[3:, 3:] = RE, J
    return e, A, B


def linearize(poses, edges):
    """PG.linearize over the log above -> e (m, 6), blocks (m, 120), chi2 (m,)"""
    m = len(edges)
    e, blocks, chi2 = np.zeros((m, 6)), np.zeros((m, 120)), np.zeros(m)
    for k, (a, b, Z, W) in enumerate(edges):
        ek, A, B = edge_jacobians(poses[a], poses[b], Z)
        e[k] = ek
        blocks[k] = np.concatenate([(A.T @ W @ A).ravel(), (A.T @ W @ B).ravel(), (B.T @ W @ B).ravel(), A.T @ W @ ek, B.T @ W @ ek])
        chi2[k] = ek @ W @ ek
    return e, blocks, chi2


class Robust:
    """what lsa_pgo_robust_t and the edge mask say, for the numpy side"""

    def __init__(self, edge_loss=NONE, edge_scale=1.0, prior_loss=NONE, prior_scale=1.0, mask=None):
        self.edge_loss, self.edge_scale, self.prior_loss, self.prior_scale, self.mask = edge_loss, edge_scale, prior_loss, prior_scale, mask

    def of_edge(self, k):
        return self.edge_loss if self.mask is None or self.mask[k] else NONE


def verdicts(poses, edges, priors, O, rb):
    """-> (m, 2), (k, 2): {chi2, w} of every constraint at poses"""
    _, _, chi2 = linearize(poses, edges)
    ev = np.array([[s, rho_w(rb.of_edge(k), rb.edge_scale, s)[1]] for k, s in enumerate(chi2)]).reshape(-1, 2)
    pchi2 = PP.linearize_priors(poses, priors, O)[2] if len(priors) else np.zeros(0)
    pv = np.array([[s, rho_w(rb.prior_loss, rb.prior_scale, s)[1]] for s in pchi2]).reshape(-1, 2)
    return ev, pv


def cost(poses, edges, priors, O, rb):
    _, _, chi2 = linearize(poses, edges)
    F = sum(rho_w(rb.of_edge(k), rb.edge_scale, s)[0] for k, s in enumerate(chi2))
    if len(priors):
        F += sum(rho_w(rb.prior_loss, rb.prior_scale, s)[0] for s in PP.linearize_priors(poses, priors, O)[2])
    return 0.5 * F


def dense_system(poses, fixed, edges, priors, O, rb, lam=0.0):
    """PP.dense_system over the weighted block records: H_lambda, g, diag(H) undamped"""
    n = len(poses)
    H, g = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    _, blocks, chi2 = linearize(poses, edges)
    for k, (a, b, _, _) in enumerate(edges):
        w = rho_w(rb.of_edge(k), rb.edge_scale, chi2[k])[1]
        blk = w * blocks[k]
        sa, sb = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
        Hab = blk[36:72].reshape(6, 6)
        H[sa, sa] += blk[:36].reshape(6, 6)
        H[sb, sb] += blk[72:108].reshape(6, 6)
        H[sa, sb] += Hab
        H[sb, sa] += Hab.T
        g[sa] += blk[108:114]
        g[sb] += blk[114:120]
    if len(priors):
        _, pblocks, pchi2 = PP.linearize_priors(poses, priors, O)
        for a, (i, _, _) in enumerate(priors):
            w = rho_w(rb.prior_loss, rb.prior_scale, pchi2[a])[1]
            s = slice(6 * i, 6 * i + 6)
            H[s, s] += w * pblocks[a, :36].reshape(6, 6)
            g[s] += w * pblocks[a, 36:]
    for i in range(n):
        if fixed[i]:
            s = slice(6 * i, 6 * i + 6)
            H[s, :] = 0.0
            H[:, s] = 0.0
            g[s] = 0.0
    dg = np.diag(H).copy()
    H[np.diag_indices(6 * n)] += lam * dg
    for i in range(n):
        if fixed[i]:
            H[6 * i : 6 * i + 6, 6 * i : 6 * i + 6] = np.eye(6)
    return H, g, dg


def dense_lm(poses, fixed, edges, priors, O, p, rb):
    """The LM loop of lsa_pose_graph.h under losses, with a dense direct solve in PCG's place.
    -> poses, final cost, initial cost, termination, iterations"""
    x = [np.array(T, np.float64) for T in poses]
    n = len(x)
    F = cost(x, edges, priors, O, rb)
    F0, lam, term, its = F, p.initial_lambda, 0, 0
    for _ in range(p.max_iterations):
        its += 1
        H, g, dg = dense_system(x, fixed, edges, priors, O, rb, lam)
        if np.abs(g).max() <= p.gradient_tolerance:
            term = 1
            break
        delta = np.linalg.solve(H, -g)
        step = np.abs(delta).max()
        model = 0.5 * float(delta @ (lam * dg * delta - g))
        cand = [PG.retract(x[i], delta[6 * i : 6 * i + 6]) for i in range(n)]
        Fn = cost(cand, edges, priors, O, rb)
        if model > 0 and np.isfinite(Fn) and F - Fn > 0:
            small = (F - Fn) <= p.cost_tolerance * F
            x, F = cand, Fn
            lam = max(lam * p.lambda_shrink, p.lambda_min)
            if step <= p.step_tolerance:
                term = 2
                break
            if small:
                term = 3
                break
        else:
            lam *= p.lambda_grow
            if step <= p.step_tolerance:
                term = 2
                break
            if lam > p.lambda_max:
                term = 4
                break
    return np.array(x), F, F0, term, its


# ---- the graphs --------------------------------------------------------------------------------------------------------------
# Odometry of 2 mm / 0.2 mrad a step; a loop edge as a cautious registration gives it, 0.5 m / 0.1 rad.  The drift of a lap stays a
# fraction of a loop sigma, so every true loop starts with chi2 < c2 / 4 at SCALE; a false loop is a true one moved by
# FALSE_OFFSET metres (a wrong place across the street), hundreds of its sigmas: chi2 > 100 c2 wherever the solve goes.
SCALE = 3.0
ODOMETRY_SIGMA = np.array([0.002] * 3 + [0.0002] * 3)
LOOP_SIGMA = np.array([0.5] * 3 + [0.1] * 3)
W_ODOMETRY = np.diag(1.0 / ODOMETRY_SIGMA**2)
W_LOOP = np.diag(1.0 / LOOP_SIGMA**2)
FALSE_OFFSET = 50.0
TRUE_LOOPS = {16: [(2, 15)], 64: [(3, 63)], 200: [(1, 199), (10, 150), (50, 120)]}
FALSE_LOOPS = {16: [(4, 11)], 64: [(10, 40)], 200: [(30, 170), (90, 20)]}
# five true and two false loops (the device tests)
TRUE_LOOPS_MANY = {64: [(3, 63), (5, 40), (12, 50), (20, 58), (30, 8)], 257: [(2, 256), (3, 250), (40, 140), (100, 200), (128, 5)],
                   1000: [(1, 999), (10, 900), (250, 750), (400, 420), (600, 100)]}
FALSE_LOOPS_MANY = {64: [(10, 45), (55, 25)], 257: [(20, 220), (180, 60)], 1000: [(50, 700), (850, 300)]}


def moved(Z, offset):
    out = Z.copy()
    out[:3, 3] += offset
    return out


@functools.lru_cache(maxsize=None)
def robust_graph(n, with_false=True, many=False, offset=FALSE_OFFSET):
    """A lap of n poses, pose 0 fixed: the odometry chain, TRUE_LOOPS[n] and (with_false) FALSE_LOOPS[n] (many: the _MANY
    lists), true and false loops interleaved -> (initial poses, fixed, edges, mask (1 on every loop edge), is_false (m,) flags,
    truth).  The chain does not depend on with_false: without the false loops it is the same graph less those edges."""
    rng = np.random.default_rng(9000 + n)
    truth = [PG.circle_pose(2 * np.pi * i / max(n, 16), i) for i in range(n)]
    edges, init = [], [truth[0]]
    for i in range(1, n):
        Z = PG.retract(np.linalg.inv(truth[i - 1]) @ truth[i], ODOMETRY_SIGMA * rng.standard_normal(6))
        edges.append((i - 1, i, Z, W_ODOMETRY))
        init.append(init[-1] @ Z)
    loops = [(a, b, False) for a, b in (TRUE_LOOPS_MANY if many else TRUE_LOOPS)[n]]
    if with_false:
        for k, (a, b) in enumerate((FALSE_LOOPS_MANY if many else FALSE_LOOPS)[n]):
            loops.insert(2 * k + 1, (a, b, True))
    false = [False] * (n - 1)
    for k, (a, b, bad) in enumerate(loops):
        Z = np.linalg.inv(truth[a]) @ truth[b]
        if bad:
            Z = moved(Z, offset * np.array([0.6, -0.8, 0.0]) * (1.0 + 0.2 * k))
        edges.append((a, b, Z, W_LOOP))
        false.append(bad)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    mask = np.array([0] * (n - 1) + [1] * len(loops), np.uint8)
    return np.array(init), fixed, edges, mask, np.array(false), np.array(truth)


GPS_SIGMA = 0.5


@functools.lru_cache(maxsize=None)
def robust_gps_graph(n, s, outliers=(2,), with_false=False, many=False, offset=FALSE_OFFSET, fix_first=False):
    """robust_graph(n, with_false, many) with every pose free and a position prior at every s-th pose behind PP.lever_arm(): fixes
    of 0.1 m noise weighted as 0.5 m, the fixes listed in `outliers` (indices into the priors) `offset` metres off, as the
    false loops are.  The start is the odometry chain in the fixes' frame; fix_first: pose 0 is held there.  -> (start, fixed, edges, mask, priors, O, is_outlier (k,), is_false (m,))"""
    init, fixed, edges, mask, false, truth = robust_graph(n, with_false, many, offset)
    Wt, O = PP.world_transform(), PP.lever_arm()
    rng = np.random.default_rng(9500 + n)
    W = np.eye(3) / GPS_SIGMA**2
    priors = [(i, (Wt @ truth[i] @ O)[:3, 3] + 0.1 * rng.standard_normal(3), W) for i in range(0, n, s)]
    bad = np.zeros(len(priors), bool)
    for a in outliers:
        i, g, _ = priors[a]
        priors[a] = (i, g + offset * np.array([0.0, 0.6, 0.8]), W)
        bad[a] = True
    return np.array([Wt @ T for T in init]), fixed if fix_first else np.zeros(n, np.uint8), edges, mask, priors, O, bad, false
