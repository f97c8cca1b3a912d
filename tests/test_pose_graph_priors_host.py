"""Position priors in the host statement of the pose-graph solve (lidarslam_amd/csrc/host/lsa_pose_graph.cpp over
lsa_pose_graph.h), the GPS matcher and the track alignment (host/lsa_gps.cpp) against independent numpy statements
(tests/pose_graph_prior_cases.py).  No GPU."""
import ctypes as C
import os
import platform
import shutil
import subprocess

import numpy as np
import pytest

import pose_graph_cases as PG
import pose_graph_prior_cases as PP
from conftest import bits, pose_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, rel=1e-12):
    """relative to the largest entry of the reference array (the bound of tests/test_pose_graph_host.py)"""
    return np.abs(a - b).max() <= rel * np.abs(b).max()


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))


def test_prior_jacobian_equals_central_differences_of_the_numpy_statement(L):
    """h = 1e-6: truncation h^2 |e'''| / 6 ~ 1e-12 times the lever arm, rounding eps |e| / h ~ 1e-9 at errors of metres: 2e-6
    holds both with room, as for the edges; the analytic Jacobians of the C++ and of numpy must agree to 1e-10."""
    poses, _, _ = PG.feature_graph()
    priors, O = PP.feature_priors()
    W = np.eye(3)
    cases = [(i, g, O) for i, g, _ in priors]
    cases += [(2, (poses[2] @ O)[:3, 3] + [30.0, -20.0, 5.0], O)]  # tens of metres off
    cases += [(4, poses[4][:3, 3] + 1e-9, O), (4, poses[4][:3, 3].copy(), O)]  # d next to zero and zero
    cases += [(1, poses[1][:3, 3] + [0.3, 0.1, -0.2], np.eye(4)), (6, poses[6][:3, 3].copy(), np.eye(4))]  # no lever arm; nothing at all
    for i, g, off in cases:
        e, A = L.pose_graph_prior_jacobian(poses, (i, g, W), off)
        e_np, A_np = PP.prior_jacobian(poses[i], off, g)
        An = PP.numeric_prior_jacobian(poses[i], off, g)
        assert np.abs(e - e_np).max() <= 1e-12 * max(1.0, np.abs(e_np).max())
        assert np.abs(A - A_np).max() <= 1e-10
        assert np.abs(A - An).max() <= 2e-6 * max(1.0, np.abs(An).max()), np.abs(A - An).max()


def test_linearize_priors_host_against_numpy(L):
    poses, _, _ = PG.feature_graph()
    priors, O = PP.feature_priors()
    e, blocks, chi2 = L.pose_graph_linearize_priors(poses, priors, O)
    e_np, blocks_np, chi2_np = PP.linearize_priors(poses, priors, O)
    assert chi2_np.min() > 1e-3  # no error vanishes
    assert close(e, e_np) and close(chi2, chi2_np)
    assert close(blocks[:, :36], blocks_np[:, :36]) and close(blocks[:, 36:], blocks_np[:, 36:])


@pytest.mark.parametrize("lam", [0.0, 1e-3, 2.0])
def test_assemble_with_priors_host_against_numpy(L, lam):
    poses, fixed, edges = PG.feature_graph()
    priors, O = PP.feature_priors()
    per_pose = np.bincount([i for i, _, _ in priors], minlength=len(poses))
    assert sorted(set(per_pose)) == [0, 1, 3] and per_pose[0] == per_pose[-1] == 1 and fixed[0] and fixed[3] and per_pose[3] == 1
    D, g, Lo, U = L.pose_graph_assemble(poses, fixed, edges, lam, priors=priors, offset=O)
    H, g_np, _ = PP.dense_system(poses, fixed, edges, priors, O, lam)
    D_np, L_np, U_np = PG.tridiagonal_of(H, len(poses))
    assert close(D, D_np) and close(g, g_np.reshape(-1, 6)) and close(Lo, L_np) and close(U, U_np)
    # the priors reach the diagonal blocks and the gradient of their free poses and nothing else
    D0, g0, L0, U0 = L.pose_graph_assemble(poses, fixed, edges, lam)
    assert same_bits(Lo, L0) and same_bits(U, U0)
    for i in range(len(poses)):
        changed = not same_bits(D[i], D0[i])
        assert changed == (per_pose[i] > 0 and not fixed[i]), i
        assert changed == (not same_bits(g[i], g0[i]))
    for i in np.flatnonzero(fixed):
        assert np.array_equal(D[i], np.eye(6)) and not g[i].any()
    rng = np.random.default_rng(3)
    p = rng.standard_normal((len(poses), 6))
    p[fixed != 0] = 0.0
    q = L.pose_graph_spmv(poses, fixed, edges, lam, p, priors=priors, offset=O)
    assert close(q, (H @ p.ravel()).reshape(-1, 6))


def test_a_prior_on_a_fixed_pose_counts_in_the_cost_alone(L):
    poses, fixed, edges = PG.feature_graph()
    priors, O = PP.feature_priors()
    on_fixed = [pr for pr in priors if fixed[pr[0]]]
    free = [pr for pr in priors if not fixed[pr[0]]]
    assert len(on_fixed) == 2
    _, r_all = L.pose_graph_solve_host(poses, fixed, edges, priors=free + on_fixed, offset=O, max_iterations=0)
    _, r_free = L.pose_graph_solve_host(poses, fixed, edges, priors=free, offset=O, max_iterations=0)
    extra = 0.5 * PP.linearize_priors(poses, on_fixed, O)[2].sum()
    assert extra > 1e-3 and abs(r_all.initial_cost - r_free.initial_cost - extra) <= 1e-12 * r_all.initial_cost
    assert same_bits(L.pose_graph_assemble(poses, fixed, edges, 0.1, priors=free + on_fixed, offset=O)[0],
                     L.pose_graph_assemble(poses, fixed, edges, 0.1, priors=free, offset=O)[0])


def check_solve(L, start, fixed, edges, priors, O, n):
    p = L.PoseGraphParams()
    out, res = L.pose_graph_solve_host(start, fixed, edges, params=p, priors=priors, offset=O)
    ref, F_ref, F0_ref, term_ref, its_ref = PP.dense_lm(start, fixed, edges, priors, O, p)
    dpos = max(pose_diff(ref[i], out[i])[0] for i in range(n))
    drot = max(pose_diff(ref[i], out[i])[1] for i in range(n))
    print(f"n {n}, {len(priors)} priors: {res.iterations} LM iterations (numpy {its_ref}), {res.pcg_iterations} PCG iterations, termination {res.termination} "
          f"(numpy {term_ref}); against numpy {dpos:.2e} m {drot:.2e} rad, cost {res.initial_cost:.4g} -> {res.final_cost:.6g} (rel {abs(res.final_cost - F_ref) / F_ref:.1e})")
    assert res.termination in (L.PGO_GRADIENT, L.PGO_STEP, L.PGO_COST) and res.termination == term_ref
    assert abs(res.initial_cost - F0_ref) <= 1e-12 * F0_ref
    assert dpos <= 1e-8 and drot <= 1e-7
    assert abs(res.final_cost - F_ref) <= 1e-9 * F_ref
    assert res.pcg_truncated == 0 and res.accepted_steps >= 1
    return out, res


@pytest.mark.parametrize("n,s", PP.CASES)
def test_solve_with_priors_host_against_a_dense_numpy_lm(L, n, s):
    init, aligned, fixed, edges, priors, O, truth = PP.gps_case(n, s)
    assert not fixed.any()
    out, res = check_solve(L, aligned, fixed, edges, priors, O, n)
    assert res.final_cost < res.initial_cost
    # the fixes hold the track where they say it is: within a few of their 0.03 m of the truth in their frame
    assert max(float(np.linalg.norm(out[i][:3, 3] - truth[i][:3, 3])) for i in range(n)) < 0.5
    # from the odometry chain where it was logged (100 m and 0.8 rad away) the same minimum: 1e-7 m, what the issue's dense runs
    # gave at n = 3 (3.4e-8 m) with room, a tenth of a micrometre
    far, res_far = L.pose_graph_solve_host(init, fixed, edges, priors=priors, offset=O)
    assert res_far.termination in (L.PGO_GRADIENT, L.PGO_STEP, L.PGO_COST)
    assert max(pose_diff(out[i], far[i])[0] for i in range(n)) <= 1e-7


def test_solve_two_poses_with_the_first_fixed(L):
    init, aligned, fixed, edges, priors, O, _ = PP.gps_case(2, 1)
    fixed = fixed.copy()
    fixed[0] = 1
    out, _ = check_solve(L, aligned, fixed, edges, priors, O, 2)
    assert np.array_equal(out[0], aligned[0])


def raw_solve(L, poses, fixed, edges, priors, O, k=None, plain=False):
    P = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 16))
    E = L.pose_graph_edges(edges)
    R = L.pose_graph_priors(priors)
    Om = np.ascontiguousarray(np.asarray(O, np.float64).reshape(16))
    f = np.ascontiguousarray(fixed, np.uint8)
    out = np.full_like(P, -7.0)
    r = L.PoseGraphResultStruct()
    r.iterations = -7
    p = L.PoseGraphParams()
    if plain:
        rc = L.lib().lsa_pgo_solve_host(L.ptr(P), P.shape[0], L.ptr(f), L.ptr(E), E.size, C.byref(p), L.ptr(out), C.byref(r))
    else:
        rc = L.lib().lsa_pgo_solve_priors_host(L.ptr(P), P.shape[0], L.ptr(f), L.ptr(E), E.size, L.ptr(R) if R.size else None, R.size if k is None else k, L.ptr(Om),
                                               C.byref(p), L.ptr(out), C.byref(r))
    return rc, out, r


@pytest.mark.parametrize("graph", ["features", 64])
def test_no_prior_gives_the_bits_of_the_solve_without_priors(L, graph):
    poses, fixed, edges = PG.feature_graph() if graph == "features" else PG.circle_graph(64)[:3]
    rc0, out0, r0 = raw_solve(L, poses, fixed, edges, [], np.eye(4), plain=True)
    rc1, out1, r1 = raw_solve(L, poses, fixed, edges, [], np.eye(4))
    assert rc0 == rc1 == 0 and same_bits(out0, out1) and r0.iterations > 0
    for name, _ in L.PoseGraphResultStruct._fields_:
        a, b = getattr(r0, name), getattr(r1, name)
        assert (same_bits(a, b) if isinstance(a, float) else a == b), name
    for lam in (0.0, 0.37):
        for h, d in zip(L.pose_graph_assemble(poses, fixed, edges, lam), L.pose_graph_assemble(poses, fixed, edges, lam, priors=[], offset=np.eye(4))):
            assert same_bits(h, d)


def test_solve_with_priors_refusals_leave_the_output_untouched(L):
    init, aligned, fixed, edges, priors, O, _ = PP.gps_case(16, 3)

    def refused(P, f, E, R, k=None):
        rc, out, r = raw_solve(L, P, f, E, R, O, k)
        assert rc == L.E_ARG and np.all(out == -7.0) and r.iterations == -7

    refused(aligned, fixed, edges, [])  # no fixed pose and no prior
    with pytest.raises(L.LsaError):
        L.pose_graph_solve_host(aligned, fixed, edges, priors=[], offset=O)
    refused(aligned, fixed, edges, priors + [(16, np.zeros(3), np.eye(3))])  # index n
    refused(aligned, fixed, edges, priors + [(-1, np.zeros(3), np.eye(3))])
    refused(aligned, fixed, edges, priors + [(3, np.array([0.0, np.nan, 0.0]), np.eye(3))])
    refused(aligned, fixed, edges, priors + [(3, np.zeros(3), np.diag([1.0, np.inf, 1.0]))])
    refused(aligned, fixed, edges, priors, k=-1)
    refused(aligned, fixed, [e for e in edges if 7 not in (e[0], e[1])], priors + [(7, np.zeros(3), np.eye(3))])  # priors alone do not hold a pose
    bad = O.copy()
    bad[1, 3] = np.nan
    rc, out, _ = raw_solve(L, aligned, fixed, edges, priors, bad)
    assert rc == L.E_ARG and np.all(out == -7.0)
    # an indefinite information is the caller's: the solver takes it and ends by a rule; the covariance helper refuses it
    rc, out, r = raw_solve(L, aligned, fixed, edges, priors + [(5, priors[1][1], np.diag([1.0, -1e-3, 1.0]))], O)
    assert rc == 0 and np.isfinite(out).all() and 0 <= r.termination <= 5
    rc, out, _ = raw_solve(L, aligned, fixed, edges, priors, O)
    assert rc == 0 and np.isfinite(out).all()


def test_information_from_covariance3(L):
    rng = np.random.default_rng(12)
    for k in range(20):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        w = 10.0 ** rng.uniform(-4 + (k % 3), k % 3, 3)  # condition <= 1e4
        cov = (Q * w) @ Q.T
        cov = 0.5 * (cov + cov.T)
        info = L.information_from_covariance3(cov)
        ref = np.linalg.inv(cov)
        assert np.abs(info - ref).max() <= 1e-9 * np.abs(ref).max()
        assert np.array_equal(info, info.T)
    v = np.ones(3)
    asymmetric = np.eye(3)
    asymmetric[0, 1] = 0.3
    for bad in (np.diag([1.0, -1e-3, 1.0]), np.eye(3) - np.outer(v, v) / 3.0, np.zeros((3, 3)), asymmetric, np.full((3, 3), np.nan)):
        out = np.full((3, 3), -7.0)
        assert L.lib().lsa_pgo_information_from_covariance3(L.ptr(np.ascontiguousarray(bad)), L.ptr(out)) == L.E_ARG
        assert np.all(out == -7.0)
        with pytest.raises(L.LsaError):
            L.information_from_covariance3(bad)


def match_by_brute_force(slam, gps, offset, bound):
    """the rule, stated over all pairs: nearest in time within the bound, the earlier of two equally near; no pose twice in a row"""
    out, previous = [], -1
    for t in gps:
        d = np.abs(t - (np.asarray(slam) + offset))
        j = int(np.argmin(d)) if d.size else -1  # argmin: the first of equal minima
        if j >= 0 and d[j] <= bound and j != previous:
            previous = j
            out.append(j)
        else:
            out.append(-1)
    return np.array(out, np.int32)


def test_gps_match_trajectory_against_brute_force(L):
    slam = 100.0 + 0.1 * np.arange(40)  # 10 Hz
    rng = np.random.default_rng(21)
    dense = np.sort(100.0 + 4.2 * rng.random(300) - 0.15)  # denser than the poses, some before the first and after the last
    sparse = 100.0 + 0.73 * np.arange(6) + 0.004
    # halves and quarters of a second are exact in binary: 10.25 lies exactly between 10.0 and 10.5, 12.625 is 0.125 after 12.5
    grid = 10.0 + 0.5 * np.arange(8)
    exact = np.array([10.25, 11.0, 12.625, 12.626])
    cases = [(slam, dense, 0.0, 0.1), (slam, sparse, 0.0, 0.1), (grid, exact, 0.0, 0.25), (grid, exact, 0.0, 0.125), (grid, exact, 0.0, 0.125 - 1e-9),
             (np.array([0.0, 1.0]), np.array([0.1, 1.1 + 1e-9]), 0.0, 0.1), (np.array([0.0, 1.0]), np.array([-0.1, 0.9 - 1e-9]), 0.0, 0.1),
             (slam - 37.5, dense, 37.5, 0.1), (slam, sparse + 0.05, -0.05, 0.02), (slam, np.array([]), 0.0, 0.1), (np.array([]), sparse, 0.0, 0.1)]
    for s, g, off, bound in cases:
        got = L.gps_match_trajectory(s, g, off, bound)
        ref = match_by_brute_force(s, g, off, bound)
        assert np.array_equal(got, ref), (s[:4], g[:6], off, bound, got, ref)
    got = L.gps_match_trajectory(slam, dense)
    assert (got >= 0).sum() >= 38 and (got == -1).sum() > 200  # the dedup at work
    assert list(L.gps_match_trajectory(grid, exact, 0.0, 0.25)) == [0, 2, 5, -1]  # the tie goes to the earlier pose; 12.626 meets pose 5 again
    assert list(L.gps_match_trajectory(np.array([0.0, 1.0]), np.array([0.1, 1.1 + 1e-9]))) == [0, -1]  # 0.1 s off is inside, a nanosecond more is not
    with pytest.raises(L.LsaError):
        L.gps_match_trajectory(slam[::-1], sparse)
    with pytest.raises(L.LsaError):
        L.gps_match_trajectory(slam, np.array([1.0, np.nan]))


def horn_gap(a, b):
    """the gap between the two largest eigenvalues of Horn's matrix over the largest"""
    a, b = a - a.mean(0), b - b.mean(0)
    S = a.T @ b
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    w = np.linalg.eigvalsh(N)
    return (w[3] - w[2]) / w[3]


@pytest.mark.parametrize("track", ["helix", "circle", "three"])
def test_trajectory_alignment_against_kabsch(L, track):
    """1e-10 rad and 1e-10 x the track's extent: the eigenvector of a symmetric matrix moves by eps / gap, 2e-14 with the gap of
    1e-2 asserted here, four orders inside the bound"""
    rng = np.random.default_rng(31)
    s = np.linspace(0.0, 4 * np.pi, 60)
    if track == "helix":
        a = np.stack([15 * np.cos(s), 15 * np.sin(s), 0.8 * s], axis=1)
    elif track == "circle":
        a = np.stack([15 * np.cos(s), 15 * np.sin(s), 0 * s], axis=1)  # rank 2
    else:
        a = np.array([[0.0, 0.0, 0.0], [12.0, 1.0, 0.5], [5.0, 9.0, -1.0]])
    Wt = PP.world_transform()
    b = a @ Wt[:3, :3].T + Wt[:3, 3] + 0.02 * rng.standard_normal(a.shape)
    assert horn_gap(a, b) >= 1e-2
    T = L.trajectory_alignment(a, b)
    ref = PP.kabsch(a, b)
    extent = float(np.abs(a - a.mean(0)).max())
    assert np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]) and abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
    drot = pose_diff(ref, T)[1]
    dpos = float(np.abs((a @ T[:3, :3].T + T[:3, 3]) - (a @ ref[:3, :3].T + ref[:3, 3])).max())
    print(f"{track}: against Kabsch {drot:.2e} rad, {dpos:.2e} m over an extent of {extent:.1f} m")
    # (arccos resolves angles down to sqrt(eps) only: the rotation is compared entry by entry)
    assert np.abs(T[:3, :3] - ref[:3, :3]).max() <= 1e-10 and dpos <= 1e-10 * extent


def rough_estimate(a, b):
    """GlobalTrajectoriesRegistration's rough estimate: the translation first -> first and the least rotation carrying the chord
    first -> last of a onto that of b, composed as translation * rotation"""
    T = np.eye(4)
    T[:3, 3] = b[0] - a[0]
    u, v = a[-1] - a[0], b[-1] - b[0]
    if np.linalg.norm(u) > 0 and np.linalg.norm(v) > 0:
        u, v = u / np.linalg.norm(u), v / np.linalg.norm(v)
        axis = np.cross(u, v)
        sn, cs = np.linalg.norm(axis), float(u @ v)
        if sn > 0:
            T[:3, :3] = PG.exp_so3(axis / sn * np.arctan2(sn, cs))
    return T


def test_trajectory_alignment_of_collinear_tracks_is_the_rough_estimate(L):
    s = np.linspace(0.0, 30.0, 25)[:, None]
    a = np.array([1.0, 2.0, -0.5]) + s * np.array([0.6, 0.0, 0.8])
    Wt = PP.world_transform()
    b = a @ Wt[:3, :3].T + Wt[:3, 3]
    for aa, bb in ((a, b), (a[:2], b[:2]), (a[:1], b[:1]), (np.repeat(a[:1], 4, 0), b[:4])):
        T = L.trajectory_alignment(aa, bb)
        ref = rough_estimate(aa, bb)
        assert np.abs(T - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (len(aa), T, ref)
    # the chord of a is carried onto the chord of b
    T = L.trajectory_alignment(a, b)
    u, v = T[:3, :3] @ (a[-1] - a[0]), b[-1] - b[0]
    assert np.linalg.norm(np.cross(u, v)) <= 1e-9 * np.linalg.norm(u) * np.linalg.norm(v) and u @ v > 0
    with pytest.raises(L.LsaError):
        L.trajectory_alignment(np.zeros((0, 3)), np.zeros((0, 3)))


def test_transforms_host_against_numpy(L):
    poses, _, _, _ = PG.circle_graph(16)
    Wt = PP.world_transform()
    out = L.pose_graph_premultiply(poses, Wt)
    assert np.abs(out - np.array([Wt @ T for T in poses])).max() <= 1e-12 * 120.0
    back = L.pose_graph_reanchor(out)
    ref = np.array([np.linalg.inv(poses[0]) @ T for T in poses])
    assert np.abs(back - ref).max() <= 1e-12 * 120.0
    assert np.abs(back[0] - np.eye(4)).max() <= 4 * PG.EPS


def test_host_statement_with_priors_under_the_sanitizers(tmp_path):
    """tests/pose_graph_prior_sanitize.cpp: the host statement with priors, the matcher and the alignment with their own main
    under -fsanitize=address,undefined, built and run the way tests/test_host_pose_graph.py does"""
    host = os.path.join(ROOT, "lidarslam_amd", "csrc", "host")
    exe = str(tmp_path / "pose_graph_prior_sanitize")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags + ["-I" + host, os.path.join(ROOT, "tests", "pose_graph_prior_sanitize.cpp"),
                                                                             os.path.join(host, "lsa_pose_graph.cpp"), os.path.join(host, "lsa_gps.cpp"), "-o", exe]
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
