"""The host statement of the pose-graph solve (lidarslam_amd/csrc/host/lsa_pose_graph.cpp over lsa_pose_graph.h) against an
independent numpy statement (tests/pose_graph_cases.py) and, for Log / Exp / Jr^-1, against mpmath.  No GPU."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import pose_graph_cases as PG
from conftest import pose_diff

EPS = PG.EPS
THETAS = [0.0, 1e-12, 1e-8, 1e-4, 1e-2, 1.0, 3.0, float(np.pi) - 1e-3]
AXES = [np.array([0.36, -0.48, 0.8]), np.array([-0.6, 0.0, 0.8]), np.array([1.0, 0.0, 0.0]), np.array([2.0, 3.0, -6.0]) / 7.0]


def mp_hat(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def mp_exp(phi):
    th = mp.sqrt(sum(x * x for x in phi))
    S = mp_hat(phi)
    if th == 0:
        return mp.eye(3)
    return mp.eye(3) + mp.sin(th) / th * S + (1 - mp.cos(th)) / th**2 * S * S


def mp_jr_inv(phi):
    th = mp.sqrt(sum(x * x for x in phi))
    S = mp_hat(phi)
    c = mp.mpf(1) / 12 if th == 0 else 1 / th**2 - (1 + mp.cos(th)) / (2 * th * mp.sin(th))
    return mp.eye(3) + S / 2 + c * S * S


def to_np(M):
    return np.array([[float(M[i, j]) for j in range(3)] for i in range(3)])


def pose_of(R):
    T = np.eye(4)
    T[:3, :3] = R
    return T


@pytest.mark.parametrize("theta", THETAS)
def test_exp_log_and_the_inverse_right_jacobian_against_mpmath(L, theta):
    """Bound per entry: 16 eps (|reference| + theta) for Exp and Log, twice that for Jr^-1.  Exp = I + a [phi]x + b [phi]x^2:
    a [phi]x carries sin, a division and a product (3 roundings of something of size theta), b [phi]x^2 two sines, a division,
    a two-term sum and two products (7 roundings of something of size theta^2 / 2 <= 1.6 theta), the last addition one rounding
    of the entry itself.  Log sees a matrix rounded to double (each entry off by eps of itself: the sine part by eps theta, the
    diagonal by eps, which reaches phi only through w = sqrt(1 + trace) / 2, relatively), then a square root, a division, atan2
    and a product: again a handful of roundings of something of size theta; next to pi, where the quaternion's vector part
    comes from sums of entries of size 1, their eps is eps theta / 3 as well.  Jr^-1 is evaluated at the Log just computed
    (within the bound above of phi, and Jr^-1 moves half as fast as phi) and its coefficient c is a quotient of quantities of
    size theta^2 / 12 with errors of 3 eps max(1, theta^2 / 12): twice the bound.  theta = 0 must be exact."""
    mp.mp.dps = 60
    worst = [0.0, 0.0, 0.0]
    for axis in AXES:
        phi = theta * axis
        th = float(np.linalg.norm(phi))
        mphi = [mp.mpf(float(x)) for x in phi]
        R_ref, J_ref = mp_exp(mphi), mp_jr_inv(mphi)
        # Exp through the retraction of the identity
        R = L.pose_graph_retract(np.eye(4)[None], np.concatenate([np.zeros(3), phi])[None])[0][:3, :3]
        for i in range(3):
            for j in range(3):
                bound = 16 * EPS * (abs(float(R_ref[i, j])) + th)
                err = abs(float(mp.mpf(float(R[i, j])) - R_ref[i, j]))
                worst[0] = max(worst[0], err / bound if bound else err)
                assert err <= bound, ("Exp", theta, i, j, err, bound)
        # Log and Jr^-1 through an edge from the identity to (R_ref rounded, 0) measured as the identity
        Rd = to_np(R_ref)
        e, A, B = L.pose_graph_edge_jacobians(np.array([np.eye(4), pose_of(Rd)]), (0, 1, np.eye(4), np.eye(6)))
        for k in range(3):
            bound = 16 * EPS * (abs(phi[k]) + th)
            err = abs(float(mp.mpf(float(e[3 + k])) - mphi[k]))
            worst[1] = max(worst[1], err / bound if bound else err)
            assert err <= bound, ("Log", theta, k, err, bound)
        for i in range(3):
            for j in range(3):
                bound = 32 * EPS * (abs(float(J_ref[i, j])) + th)
                err = abs(float(mp.mpf(float(B[3 + i, 3 + j])) - J_ref[i, j]))
                worst[2] = max(worst[2], err / bound if bound else err)
                assert err <= bound, ("Jr^-1", theta, i, j, err, bound)
    print(f"theta {theta:g}: worst error / bound  Exp {worst[0]:.3f}  Log {worst[1]:.3f}  Jr^-1 {worst[2]:.3f}")


def test_jacobians_equal_central_differences_of_the_numpy_statement(L):
    """h = 1e-6: truncation h^2 |e'''| / 6 ~ 1e-12 times the lever arm (tens of metres), rounding eps |e| / h ~ 1e-9: 2e-6 holds
    both with room; the analytic Jacobians of the C++ and of numpy must agree far better (1e-10)."""
    poses, _, edges = PG.feature_graph()
    for a, b, Z, W in edges:
        e, A, B = L.pose_graph_edge_jacobians(poses, (a, b, Z, W))
        e_np, A_np, B_np = PG.edge_jacobians(poses[a], poses[b], Z)
        An, Bn = PG.numeric_jacobians(poses[a], poses[b], Z)
        assert np.abs(e - e_np).max() <= 1e-12 * max(1.0, np.abs(e_np).max())
        assert np.abs(A - A_np).max() <= 1e-10 and np.abs(B - B_np).max() <= 1e-10
        assert np.abs(A - An).max() <= 2e-6 * max(1.0, np.abs(An).max()), np.abs(A - An).max()
        assert np.abs(B - Bn).max() <= 2e-6 * max(1.0, np.abs(Bn).max()), np.abs(B - Bn).max()


def close(a, b, rel=1e-12):
    """relative to the largest entry of the reference array: sums of at most 8 products of O(1) terms"""
    return np.abs(a - b).max() <= rel * np.abs(b).max()


def test_linearize_host_against_numpy(L):
    poses, _, edges = PG.feature_graph()
    e, blocks, chi2 = L.pose_graph_linearize(poses, edges)
    e_np, blocks_np, chi2_np = PG.linearize(poses, edges)
    assert chi2_np.min() > 1e-3  # no error vanishes
    assert close(e, e_np) and close(chi2, chi2_np)
    for lo, hi in ((0, 36), (36, 72), (72, 108), (108, 114), (114, 120)):
        assert close(blocks[:, lo:hi], blocks_np[:, lo:hi]), (lo, hi)


@pytest.mark.parametrize("lam", [0.0, 1e-3, 2.0])
def test_assemble_host_against_numpy(L, lam):
    poses, fixed, edges = PG.feature_graph()
    D, g, Lo, U = L.pose_graph_assemble(poses, fixed, edges, lam)
    H, g_np, _ = PG.dense_system(poses, fixed, edges, lam)
    D_np, L_np, U_np = PG.tridiagonal_of(H, len(poses))
    assert close(D, D_np) and close(g, g_np.reshape(-1, 6)) and close(Lo, L_np) and close(U, U_np)
    for i in np.flatnonzero(fixed):
        assert np.array_equal(D[i], np.eye(6)) and not g[i].any() and not Lo[i].any() and not U[i].any()
        if i > 0:
            assert not U[i - 1].any()
        if i + 1 < len(poses):
            assert not Lo[i + 1].any()
    # the whole of H_lambda, the blocks beyond the chain included, through the matrix-vector product
    rng = np.random.default_rng(3)
    p = rng.standard_normal((len(poses), 6))
    p[fixed != 0] = 0.0
    q = L.pose_graph_spmv(poses, fixed, edges, lam, p)
    assert close(q, (H @ p.ravel()).reshape(-1, 6))


@pytest.mark.parametrize("n", PG.TRIDIAGONAL_SIZES)
def test_tridiagonal_solve_host_against_numpy(L, n):
    for rows in ((),) + (((0, n // 2, n - 1),) if 9 <= n <= 257 else ()):
        D, Lo, U, b, x_ref, cond = PG.tridiagonal_case(n, 0, rows)
        x = L.pose_graph_tridiagonal_solve(D, Lo, U, b)
        ratio = PG.tridiagonal_error(x, x_ref, cond)
        print(f"n {n} identity rows {rows}: cond {cond:.3g}, error / (cond eps) {ratio:.4f} (K = {PG.TRIDIAGONAL_K:.3f})")
        assert ratio <= PG.TRIDIAGONAL_K


def test_tridiagonal_solve_host_refuses_an_indefinite_block(L):
    D, Lo, U, b, _, _ = PG.tridiagonal_case(9)
    D = D.copy()
    D[4] = -D[4]
    assert L.pose_graph_tridiagonal_solve(D, Lo, U, b) is None


@pytest.mark.parametrize("n", [2, 3, 16, 64, 200])
def test_solve_host_against_a_dense_numpy_lm(L, n):
    poses, fixed, edges, _ = PG.circle_graph(n)
    p = L.PoseGraphParams()
    out, res = L.pose_graph_solve_host(poses, fixed, edges, params=p)
    ref, F_ref, F0_ref, term_ref = PG.dense_lm(poses, fixed, edges, p)
    dpos = max(pose_diff(ref[i], out[i])[0] for i in range(n))
    drot = max(pose_diff(ref[i], out[i])[1] for i in range(n))
    moved = max(float(np.linalg.norm(out[i][:3, 3] - poses[i][:3, 3])) for i in range(n))
    print(f"n {n}: {res.iterations} LM iterations ({res.accepted_steps} accepted), {res.pcg_iterations} PCG iterations, termination {res.termination} "
          f"(numpy {term_ref}); against numpy {dpos:.2e} m {drot:.2e} rad, cost {res.initial_cost:.4g} -> {res.final_cost:.6g} "
          f"(rel {abs(res.final_cost - F_ref) / F_ref:.1e}), largest pose change {moved:.3f} m")
    assert res.termination in (L.PGO_GRADIENT, L.PGO_STEP, L.PGO_COST) and res.message
    assert abs(res.initial_cost - F0_ref) <= 1e-12 * F0_ref
    # a tenth of the project's parity tolerance (1e-7 m, 1e-6 rad): the room the device solver is given on top
    assert dpos <= 1e-8 and drot <= 1e-7
    assert abs(res.final_cost - F_ref) <= 1e-9 * F_ref
    assert res.final_cost < 0.1 * res.initial_cost
    assert moved > 0.01
    assert np.array_equal(out[0], poses[0])  # the fixed pose
    assert res.pcg_truncated == 0 and res.accepted_steps >= 1 and res.largest_step > 0.0
    if n >= 16:
        assert res.pcg_iterations > res.iterations  # the loop edges are PCG's


def raw_solve(L, poses, fixed, edges, n=None, m=None):
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    E = L.pose_graph_edges(edges)
    f = np.ascontiguousarray(fixed, np.uint8)
    out = np.full_like(P, -7.0)
    r = L.PoseGraphResultStruct()
    r.iterations = -7
    p = L.PoseGraphParams()
    rc = L.lib().lsa_pgo_solve_host(L.ptr(P), P.shape[0] if n is None else n, L.ptr(f), L.ptr(E), E.size if m is None else m, C.byref(p), L.ptr(out), C.byref(r))
    return rc, out, r


def test_solve_host_refusals_leave_the_output_untouched(L):
    poses, fixed, edges, _ = PG.circle_graph(16)
    poses, fixed = poses.copy(), fixed.copy()

    def refused(P, f, E):
        rc, out, r = raw_solve(L, P, f, E)
        assert rc == L.E_ARG and np.all(out == -7.0) and r.iterations == -7
        with pytest.raises(L.LsaError):
            L.pose_graph_solve_host(P, f, E)

    refused(poses, np.zeros(16, np.uint8), edges)  # no fixed pose
    refused(poses, fixed, [e for e in edges if 7 not in (e[0], e[1])])  # free pose 7 without an edge
    refused(poses, fixed, edges + [(3, 16, np.eye(4), np.eye(6))])  # index out of range
    refused(poses, fixed, edges + [(-1, 3, np.eye(4), np.eye(6))])
    refused(poses, fixed, edges + [(3, 3, np.eye(4), np.eye(6))])  # a pose joined with itself
    bad = poses.copy()
    bad[5, 1, 3] = np.nan
    refused(bad, fixed, edges)
    Z = np.eye(4)
    Z[0, 3] = np.inf
    refused(poses, fixed, edges + [(3, 9, Z, np.eye(6))])
    W = np.eye(6)
    W[2, 4] = np.nan
    refused(poses, fixed, edges + [(3, 9, np.eye(4), W)])
    with pytest.raises(L.LsaError):
        L.pose_graph_solve_host(poses, fixed, edges, pcg_max_iter=0)
    rc, out, _ = raw_solve(L, poses, fixed, edges)
    assert rc == 0 and np.isfinite(out).all()


def test_information_from_covariance(L):
    rng = np.random.default_rng(11)
    for k in range(20):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        w = 10.0 ** rng.uniform(-4 + (k % 3), k % 3, 6)  # condition <= 1e4
        cov = (Q * w) @ Q.T
        cov = 0.5 * (cov + cov.T)
        info = L.information_from_covariance(cov)
        ref = np.linalg.inv(cov)
        assert np.abs(info - ref).max() <= 1e-9 * np.abs(ref).max()
        assert np.array_equal(info, info.T)
    indefinite = np.diag([1.0, 2.0, -1e-3, 1.0, 1.0, 1.0])
    v = np.ones(6)
    singular = np.eye(6) - np.outer(v, v) / 6.0
    asymmetric = np.eye(6)
    asymmetric[0, 1] = 0.3
    for bad in (indefinite, singular, np.zeros((6, 6)), asymmetric, np.full((6, 6), np.nan)):
        out = np.full((6, 6), -7.0)
        assert L.lib().lsa_pgo_information_from_covariance(L.ptr(np.ascontiguousarray(bad)), L.ptr(out)) == L.E_ARG
        assert np.all(out == -7.0)
        with pytest.raises(L.LsaError):
            L.information_from_covariance(bad)
