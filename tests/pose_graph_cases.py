"""The pose graph's independent statement and the graphs the tests share (tests/test_pose_graph_host.py, test_gpu_pose_graph.py).

Everything here is numpy, written from the formulas of lidarslam_amd/csrc/lsa_pose_graph.h's comment; it shares no code with
the C++.  Retraction t += R rho, R = R Exp(phi); edge (i, j, Z, W): e = [Rz^T (Ri^T (tj - ti) - tz); Log(Rz^T Ri^T Rj)].
"""
import functools
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_graph_tridiagonal.npz")

EPS = 2.0 ** -52
# Block Thomas (the host statement) on tridiagonal_case over TRIDIAGONAL_SIZES x seeds 0..2 was measured against
# numpy.linalg.solve: the worst |x - x_ref|_inf / (|x_ref|_inf cond(T) eps) was 0.344 (at n = 1; 0.27 at n = 2, 0.24 at n = 9, below
# 0.06 from n = 63 on).  K = 16 x that leaves room for the cyclic
# reduction's different elimination order (and for numpy's own error, which the same bound holds).
TRIDIAGONAL_MEASURED_RATIO = 0.344
TRIDIAGONAL_K = 16 * TRIDIAGONAL_MEASURED_RATIO
TRIDIAGONAL_SIZES = [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1000]

OMEGA = np.diag([1e4] * 3 + [2.5e5] * 3)  # 0.01 m, 0.002 rad


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(phi):
    th = float(np.linalg.norm(phi))
    S = hat(phi)
    if th < 1e-6:
        return np.eye(3) + S + 0.5 * S @ S
    return np.eye(3) + np.sin(th) / th * S + (1.0 - np.cos(th)) / th**2 * S @ S


def log_so3(R):
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # sin(theta) axis
    s, c = float(np.linalg.norm(v)), 0.5 * (np.trace(R) - 1.0)
    th = float(np.arctan2(s, c))
    if s < 1e-7 and c > 0:
        return v * (1.0 + th * th / 6.0)
    if s > 1e-4:
        return v * (th / s)
    # next to pi: the axis is the eigenvector of the symmetric part, signed by v
    w, V = np.linalg.eigh(0.5 * (R + R.T))
    a = V[:, 2]
    if np.dot(a, v) < 0:
        a = -a
    return a * th


def jr_inv(phi):
    th = float(np.linalg.norm(phi))
    S = hat(phi)
    c = 1.0 / 12.0 + th**2 / 720.0 if th < 1e-3 else 1.0 / th**2 - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))
    return np.eye(3) + 0.5 * S + c * S @ S


def retract(T, d):
    out = np.eye(4)
    out[:3, 3] = T[:3, 3] + T[:3, :3] @ d[:3]
    out[:3, :3] = T[:3, :3] @ exp_so3(d[3:])
    return out


def edge_error(Ti, Tj, Z):
    Ri, Rj, Rz = Ti[:3, :3], Tj[:3, :3], Z[:3, :3]
    d = Ri.T @ (Tj[:3, 3] - Ti[:3, 3])
    return np.concatenate([Rz.T @ (d - Z[:3, 3]), log_so3(Rz.T @ Ri.T @ Rj)])


def edge_jacobians(Ti, Tj, Z):
    Ri, Rj, Rz = Ti[:3, :3], Tj[:3, :3], Z[:3, :3]
    d = Ri.T @ (Tj[:3, 3] - Ti[:3, 3])
    Rij = Ri.T @ Rj
    RE = Rz.T @ Rij
    e = np.concatenate([Rz.T @ (d - Z[:3, 3]), log_so3(RE)])
    J = jr_inv(e[3:])
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    A[:3, :3], A[:3, 3:], A[3:, 3:] = -Rz.T, Rz.T @ hat(d), -J @ Rij.T
    B[:3, :3], B[3:, 3:] = RE, J
    return e, A, B


def numeric_jacobians(Ti, Tj, Z, h=1e-6):
    A, B = np.zeros((6, 6)), np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        A[:, k] = (edge_error(retract(Ti, d), Tj, Z) - edge_error(retract(Ti, -d), Tj, Z)) / (2 * h)
        B[:, k] = (edge_error(Ti, retract(Tj, d), Z) - edge_error(Ti, retract(Tj, -d), Z)) / (2 * h)
    return A, B


def linearize(poses, edges):
    """-> e (m, 6), blocks (m, 120), chi2 (m,) in the layout of the ABI: Haa Hab Hbb ga gb"""
    m = len(edges)
    e, blocks, chi2 = np.zeros((m, 6)), np.zeros((m, 120)), np.zeros(m)
    for k, (a, b, Z, W) in enumerate(edges):
        ek, A, B = edge_jacobians(poses[a], poses[b], Z)
        e[k] = ek
        blocks[k] = np.concatenate([(A.T @ W @ A).ravel(), (A.T @ W @ B).ravel(), (B.T @ W @ B).ravel(), A.T @ W @ ek, B.T @ W @ ek])
        chi2[k] = ek @ W @ ek
    return e, blocks, chi2


def cost(poses, edges):
    return 0.5 * sum(float(edge_error(poses[a], poses[b], Z) @ W @ edge_error(poses[a], poses[b], Z)) for a, b, Z, W in edges)


def dense_system(poses, fixed, edges, lam=0.0):
    """H_lambda (6n, 6n), g (6n,), diag(H) undamped (6n,); a fixed pose's row is the identity, its couplings dropped"""
    n = len(poses)
    H, g = np.zeros((6 * n, 6 * n)), np.zeros(6 * n)
    _, blocks, _ = linearize(poses, edges)
    for k, (a, b, _, _) in enumerate(edges):
        sa, sb = slice(6 * a, 6 * a + 6), slice(6 * b, 6 * b + 6)
        Haa, Hab, Hbb = blocks[k, :36].reshape(6, 6), blocks[k, 36:72].reshape(6, 6), blocks[k, 72:108].reshape(6, 6)
        H[sa, sa] += Haa
        H[sb, sb] += Hbb
        H[sa, sb] += Hab
        H[sb, sa] += Hab.T
        g[sa] += blocks[k, 108:114]
        g[sb] += blocks[k, 114:120]
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


def tridiagonal_of(H, n):
    """D, L, U (n, 6, 6) of a dense matrix"""
    D, Lo, U = np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for i in range(n):
        s = slice(6 * i, 6 * i + 6)
        D[i] = H[s, s]
        if i > 0:
            Lo[i] = H[s, 6 * i - 6 : 6 * i]
        if i + 1 < n:
            U[i] = H[s, 6 * i + 6 : 6 * i + 12]
    return D, Lo, U


def dense_lm(poses, fixed, edges, p):
    """The LM loop of lsa_pose_graph.h with a dense direct solve in PCG's place.  p: the PoseGraphParams in use.
    -> poses, final cost, initial cost, termination"""
    x = [np.array(T, np.float64) for T in poses]
    n = len(x)
    F = cost(x, edges)
    F0, lam, term = F, p.initial_lambda, 0
    for _ in range(p.max_iterations):
        H, g, dg = dense_system(x, fixed, edges, lam)
        if np.abs(g).max() <= p.gradient_tolerance:
            term = 1
            break
        delta = np.linalg.solve(H, -g)
        step = np.abs(delta).max()
        model = 0.5 * float(delta @ (lam * dg * delta - g))
        cand = [retract(x[i], delta[6 * i : 6 * i + 6]) for i in range(n)]
        Fn = cost(cand, edges)
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
    return np.array(x), F, F0, term


def circle_pose(a, i):
    """on a circle of 20 m, heading along the tangent, with a little roll, pitch and height so that nothing is planar"""
    T = np.eye(4)
    T[:3, :3] = exp_so3(np.array([0.0, 0.0, a + np.pi / 2])) @ exp_so3(np.array([0.03 * np.sin(3 * a), 0.02 * np.cos(2 * a), 0.0]))
    T[:3, 3] = [20.0 * np.cos(a), 20.0 * np.sin(a), 0.5 * np.sin(a) + 0.001 * i]
    return T


# (from 16 poses on no loop edge touches the fixed pose 0: its coupling would be dropped and PCG would have nothing to do)
LOOPS = {2: [(0, 1)], 3: [(0, 2)], 16: [(2, 15)], 64: [(3, 63)], 200: [(1, 199), (10, 150), (50, 120)], 257: [(2, 256), (3, 250), (40, 140), (100, 200), (128, 5)],
         1000: [(1, 999), (10, 900), (250, 750), (400, 420), (600, 100)]}


@functools.lru_cache(maxsize=None)
def circle_graph(n, seed=0, loops=None):
    """A lap of n poses with noisy odometry and true loop edges -> (initial poses (n, 4, 4), fixed (n,), edges, truth).
    Odometry noise 0.01 m / 0.002 rad with W = OMEGA (five times that below 16 poses, so that the correction is centimetres
    even with two poses); the initial poses are the odometry composed from the true pose 0, which is fixed.  A loop edge is
    the true relative pose; below 16 poses it weighs 100 x OMEGA, without which a chain of one or two edges could not
    bring the cost below a tenth: with equal weights the error is shared between two or three edges and the cost only halves."""
    rng = np.random.default_rng(1000 + 17 * n + seed)
    loops = LOOPS[n] if loops is None else list(loops)
    small = n < 16
    truth = [circle_pose(2 * np.pi * i / max(n, 16), i) for i in range(n)]
    sig = np.array([0.01] * 3 + [0.002] * 3) * (5.0 if small else 1.0)
    edges, init = [], [truth[0]]
    for i in range(1, n):
        Z = retract(np.linalg.inv(truth[i - 1]) @ truth[i], sig * rng.standard_normal(6))
        edges.append((i - 1, i, Z, OMEGA / (25.0 if small else 1.0)))
        init.append(init[-1] @ Z)
    for a, b in loops:
        edges.append((a, b, np.linalg.inv(truth[a]) @ truth[b], OMEGA * (100.0 if small else 1.0)))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return np.array(init), fixed, edges, np.array(truth)


def random_spd(rng, scale=1.0):
    M = rng.standard_normal((6, 6))
    return scale * (M @ M.T + 0.5 * np.eye(6))


@functools.lru_cache(maxsize=None)
def feature_graph():
    """Seven poses, poses 0 and 3 fixed (one at the end, one in the middle); edge 0 a loop edge listed first, edge 1 touches
    a fixed pose, edge 2 a reversed chain edge, edges 3 and 8 duplicates, edges 9 and 10 the same loop in both directions;
    full (not diagonal) information matrices; poses off the measurements, so that no error vanishes."""
    rng = np.random.default_rng(7)
    truth = [circle_pose(0.4 * i, i) for i in range(7)]
    poses = np.array([retract(T, np.array([0.05] * 3 + [0.02] * 3) * rng.standard_normal(6)) for T in truth])
    pairs = [(1, 5), (0, 1), (2, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 5), (6, 2), (2, 6)]
    edges = [(a, b, np.linalg.inv(truth[a]) @ truth[b], random_spd(rng, 100.0)) for a, b in pairs]
    fixed = np.array([1, 0, 0, 1, 0, 0, 0], np.uint8)
    return poses, fixed, edges


@functools.lru_cache(maxsize=None)
def edge_count_graph(m):
    """m edges: a lap of max(2, m) poses, m - 1 chain edges and one loop edge (m = 1, 2: chain edges alone)"""
    n = max(2, m) if m != 2 else 3
    loops = [(0, n - 1)] if m >= 3 else []
    rng = np.random.default_rng(m)
    truth = [circle_pose(2 * np.pi * i / max(n, 16), i) for i in range(n)]
    poses = np.array([retract(T, np.array([0.02] * 3 + [0.01] * 3) * rng.standard_normal(6)) for T in truth])
    edges = [(i - 1, i, np.linalg.inv(truth[i - 1]) @ truth[i], OMEGA) for i in range(1, n)] + [(a, b, np.linalg.inv(truth[a]) @ truth[b], OMEGA) for a, b in loops]
    assert len(edges) == m
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return poses, fixed, edges


def dense_of_tridiagonal(D, Lo, U):
    n = D.shape[0]
    T = np.zeros((6 * n, 6 * n))
    for i in range(n):
        T[6 * i : 6 * i + 6, 6 * i : 6 * i + 6] = D[i]
        if i > 0:
            T[6 * i : 6 * i + 6, 6 * i - 6 : 6 * i] = Lo[i]
        if i + 1 < n:
            T[6 * i : 6 * i + 6, 6 * i + 6 : 6 * i + 12] = U[i]
    return T


@functools.lru_cache(maxsize=None)
def tridiagonal_case(n, seed=0, identity_rows=()):
    """A symmetric positive definite block-tridiagonal T = sum over the chain's links of G^T W G (as a chain of edges makes
    it) plus a ridge that keeps cond(T) <= 1e6 -> D, L, U (n, 6, 6), b, x_ref = numpy.linalg.solve, cond(T) by eigvalsh.
    identity_rows: rows replaced by the identity with their couplings dropped, as fixed poses are."""
    rng = np.random.default_rng(50 + 7 * n + seed)
    D, Lo, U = np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for i in range(n):
        D[i] += 0.05 * np.eye(6)
    for i in range(1, n):
        A, B, W = rng.standard_normal((6, 6)), rng.standard_normal((6, 6)), random_spd(rng)
        D[i - 1] += A.T @ W @ A
        D[i] += B.T @ W @ B
        U[i - 1] += A.T @ W @ B
        Lo[i] += B.T @ W @ A
    if n == 1:
        D[0] += random_spd(rng)
    for i in identity_rows:
        D[i], Lo[i], U[i] = np.eye(6), 0.0, 0.0
        if i > 0:
            U[i - 1] = 0.0
        if i + 1 < n:
            Lo[i + 1] = 0.0
    b = rng.standard_normal((n, 6))
    # the dense eigenvalues and the dense solve of 6000 unknowns take ten seconds: for the large case they were recorded once
    # (record_tridiagonal_golden below) together with a digest of the matrix they belong to
    key = f"{n}_{seed}"
    if n >= 512 and not identity_rows and os.path.exists(GOLDEN):
        with np.load(GOLDEN, allow_pickle=False) as z:
            if f"x_{key}" in z.files and bytes(z[f"digest_{key}"]) == _digest(D, Lo, U, b):
                return D, Lo, U, b, z[f"x_{key}"].copy(), float(z[f"cond_{key}"])
    T = dense_of_tridiagonal(D, Lo, U)
    w = np.linalg.eigvalsh(T)
    assert w[0] > 0
    cond = float(w[-1] / w[0])
    assert cond <= 1e6, cond
    x = np.linalg.solve(T, b.ravel()).reshape(n, 6)
    return D, Lo, U, b, x, cond


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float64).tobytes())
    return h.digest()


def record_tridiagonal_golden(cases=((1000, 0),)):
    """Writes tests/golden/pose_graph_tridiagonal.npz: numpy.linalg.solve's x and cond(T) by eigvalsh of the large cases."""
    if os.path.exists(GOLDEN):
        os.remove(GOLDEN)
    tridiagonal_case.cache_clear()
    out = {}
    for n, seed in cases:
        D, Lo, U, b, x, cond = tridiagonal_case(n, seed)
        out[f"x_{n}_{seed}"], out[f"cond_{n}_{seed}"] = x, np.float64(cond)
        out[f"digest_{n}_{seed}"] = np.frombuffer(_digest(D, Lo, U, b), np.uint8)
    np.savez(GOLDEN, **out)
    tridiagonal_case.cache_clear()


def tridiagonal_error(x, x_ref, cond):
    """|x - x_ref|_inf / (|x_ref|_inf cond eps): what TRIDIAGONAL_K bounds"""
    return float(np.abs(x - x_ref).max() / (np.abs(x_ref).max() * cond * EPS))


def to_records(L, edges):
    return L.pose_graph_edges(edges)
