"""Position priors in the pose graph: the independent numpy statement and the graphs the tests share
(tests/test_pose_graph_priors_host.py, test_gpu_pose_graph_priors.py).  Extends tests/pose_graph_cases.py, whose edge
statement it uses; written from the formulas of lidarslam_amd/csrc/lsa_pose_graph.h's comment, it shares no code with the C++.

Prior (i, g, W) behind the offset O = (Ro, to):  d = Ri^T (g - ti),  e = Ro^T (d - to),  A = de/ddelta_i = [-Ro^T, Ro^T [d]x].
"""
import functools

import numpy as np

import pose_graph_cases as PG


def prior_error(Ti, O, g):
    d = Ti[:3, :3].T @ (np.asarray(g) - Ti[:3, 3])
    return O[:3, :3].T @ (d - O[:3, 3])


def prior_jacobian(Ti, O, g):
    d = Ti[:3, :3].T @ (np.asarray(g) - Ti[:3, 3])
    Ro = O[:3, :3]
    return Ro.T @ (d - O[:3, 3]), np.hstack([-Ro.T, Ro.T @ PG.hat(d)])


def numeric_prior_jacobian(Ti, O, g, h=1e-6):
    A = np.zeros((3, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        A[:, k] = (prior_error(PG.retract(Ti, d), O, g) - prior_error(PG.retract(Ti, -d), O, g)) / (2 * h)
    return A


def linearize_priors(poses, priors, O):
    """-> e (k, 3), blocks (k, 42) = Haa ga, chi2 (k,)"""
    k = len(priors)
    e, blocks, chi2 = np.zeros((k, 3)), np.zeros((k, 42)), np.zeros(k)
    for a, (i, g, W) in enumerate(priors):
        ea, A = prior_jacobian(poses[i], O, g)
        e[a] = ea
        blocks[a] = np.concatenate([(A.T @ W @ A).ravel(), A.T @ W @ ea])
        chi2[a] = ea @ W @ ea
    return e, blocks, chi2


def cost(poses, edges, priors, O):
    return PG.cost(poses, edges) + 0.5 * sum(float(prior_error(poses[i], O, g) @ W @ prior_error(poses[i], O, g)) for i, g, W in priors)


def dense_system(poses, fixed, edges, priors, O, lam=0.0):
    """PG.dense_system with the priors in the diagonal blocks and the gradient: H_lambda, g, diag(H) undamped"""
    n = len(poses)
    H, g, _ = PG.dense_system(poses, np.zeros(n, np.uint8), edges, 0.0)
    _, blocks, _ = linearize_priors(poses, priors, O)
    for a, (i, _, _) in enumerate(priors):
        s = slice(6 * i, 6 * i + 6)
        H[s, s] += blocks[a, :36].reshape(6, 6)
        g[s] += blocks[a, 36:]
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


def dense_lm(poses, fixed, edges, priors, O, p):
    """PG.dense_lm with priors -> poses, final cost, initial cost, termination, iterations"""
    x = [np.array(T, np.float64) for T in poses]
    n = len(x)
    F = cost(x, edges, priors, O)
    F0, lam, term, its = F, p.initial_lambda, 0, 0
    for _ in range(p.max_iterations):
        its += 1
        H, g, dg = dense_system(x, fixed, edges, priors, O, lam)
        if np.abs(g).max() <= p.gradient_tolerance:
            term = 1
            break
        delta = np.linalg.solve(H, -g)
        step = np.abs(delta).max()
        model = 0.5 * float(delta @ (lam * dg * delta - g))
        cand = [PG.retract(x[i], delta[6 * i : 6 * i + 6]) for i in range(n)]
        Fn = cost(cand, edges, priors, O)
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


def kabsch(a, b):
    """the rigid (4, 4) T minimising sum |T a_i - b_i|^2 by the SVD"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ca, cb = a.mean(0), b.mean(0)
    U, _, Vt = np.linalg.svd((b - cb).T @ (a - ca))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    T = np.eye(4)
    T[:3, :3] = U @ D @ Vt
    T[:3, 3] = cb - T[:3, :3] @ ca
    return T


def world_transform():
    """the frame of the measured positions: yaw 0.8 with a small tilt, translation (100, -50, 10)"""
    Wt = np.eye(4)
    Wt[:3, :3] = PG.exp_so3(np.array([0.0, 0.0, 0.8])) @ PG.exp_so3(np.array([0.02, -0.03, 0.0]))
    Wt[:3, 3] = [100.0, -50.0, 10.0]
    return Wt


def lever_arm():
    O = np.eye(4)
    O[:3, :3] = PG.exp_so3(np.array([0.1, -0.2, 0.3]))
    O[:3, 3] = [0.4, -0.3, 1.2]
    return O


SIGMA = 0.03
CASES = [(3, 1), (16, 3), (64, 4), (200, 7), (257, 9)]


@functools.lru_cache(maxsize=None)
def gps_case(n, s, loops=()):
    """PG.circle_graph(n) with every pose free and a prior at every s-th pose on (Wt truth_i O).t + 0.03 m noise, W = I / 0.03^2
    -> odometry chain (the unaligned start), aligned start (the chain laid onto the fixes by kabsch), fixed (zeros), edges,
    priors, O, truth in the fixes' frame.  loops: the loop edges of the graph (default none: the chain and the priors)."""
    init, _, edges, truth = PG.circle_graph(n, 0, tuple(loops))
    Wt, O = world_transform(), lever_arm()
    rng = np.random.default_rng(4000 + 31 * n + s)
    W = np.eye(3) / SIGMA**2
    priors = [(i, (Wt @ truth[i] @ O)[:3, 3] + SIGMA * rng.standard_normal(3), W) for i in range(0, n, s)]
    if len(priors) >= 3:
        A = kabsch([(init[i] @ O)[:3, 3] for i, _, _ in priors], [g for _, g, _ in priors])
    else:
        A = Wt
    aligned = np.array([A @ T for T in init])
    return init, aligned, np.zeros(n, np.uint8), edges, priors, O, np.array([Wt @ T for T in truth])


def random_spd3(rng, scale=1.0):
    M = rng.standard_normal((3, 3))
    return scale * (M @ M.T + 0.5 * np.eye(3))


PRIOR_POSES = [5, 1, 5, 6, 0, 5, 3]


@functools.lru_cache(maxsize=None)
def feature_priors(k=None, seed=0):
    """Priors for PG.feature_graph() (seven poses, 0 and 3 fixed): pose 5 has three priors listed between those of other poses
    (one of them before the prior of the lower-indexed pose 1), pose 1 has one, poses 2 and 4 none, the last pose 6 and the
    first, fixed pose 0 one each, the fixed pose 3 one; full information matrices; positions a few centimetres off, so that
    no error vanishes.  k: that many priors instead, their poses drawn at random.  -> priors, O"""
    poses, _, _ = PG.feature_graph()
    rng = np.random.default_rng(70 + seed + (0 if k is None else k))
    O = lever_arm()
    where = PRIOR_POSES if k is None else [int(i) for i in rng.integers(0, len(poses), k)]
    priors = [(i, (poses[i] @ O)[:3, 3] + 0.05 * rng.standard_normal(3), random_spd3(rng, 100.0)) for i in where]
    return priors, O
