"""The device pose-graph solver (lidarslam_amd/csrc/lsa_pose_graph.hip) held, seam by seam, to its host statement and to the
numpy statement of tests/pose_graph_cases.py; Slam.optimize_trajectory on a logged revisit."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cases as PG
from conftest import bits, pose_diff

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))


def graph_of(case):
    return PG.feature_graph() if case == "features" else PG.edge_count_graph(case)


@pytest.mark.parametrize("case", ["features", 1, 63, 64, 65, 257, 3000])
def test_linearize_and_assemble_equal_the_host_statement_bit_for_bit(L, gpu_ctx, case):
    poses, fixed, edges = graph_of(case)
    E = L.pose_graph_edges(edges)
    host = L.pose_graph_linearize(poses, E)
    dev = gpu_ctx.pose_graph_linearize(poses, E)
    assert len(host[2]) == len(edges) and np.abs(host[1]).max() > 0
    for h, d, name in zip(host, dev, ("e", "blocks", "chi2")):
        assert same_bits(h, d), (case, name, np.abs(h - d).max())
    for lam in (0.0, 0.37):
        host = L.pose_graph_assemble(poses, fixed, E, lam)
        dev = gpu_ctx.pose_graph_assemble(poses, fixed, E, lam)
        for h, d, name in zip(host, dev, ("D", "g", "L", "U")):
            assert same_bits(h, d), (case, lam, name, np.abs(h - d).max())
    rng = np.random.default_rng(5)
    p = rng.standard_normal((len(poses), 6))
    assert same_bits(L.pose_graph_spmv(poses, fixed, E, 0.37, p), gpu_ctx.pose_graph_spmv(poses, fixed, E, 0.37, p))


def test_retraction_equals_the_host_statement_bit_for_bit(L, gpu_ctx):
    poses, _, _, _ = PG.circle_graph(257)
    rng = np.random.default_rng(9)
    delta = rng.standard_normal((257, 6)) * np.array([1.0, 1.0, 1.0, 0.5, 0.5, 0.5])
    delta[:8, 3:] *= 10.0 ** -np.arange(1, 9)[:, None]  # down to angles where Exp takes its series
    delta[8] = 0.0
    assert same_bits(L.pose_graph_retract(poses, delta), gpu_ctx.pose_graph_retract(poses, delta))


@pytest.mark.parametrize("n", PG.TRIDIAGONAL_SIZES)
def test_cyclic_reduction_against_numpy(L, gpu_ctx, n):
    for rows in ((),) + (((0, n // 2, n - 1),) if 3 <= n <= 257 else ()):
        D, Lo, U, b, x_ref, cond = PG.tridiagonal_case(n, 0, rows)
        x = gpu_ctx.pose_graph_tridiagonal_solve(D, Lo, U, b)
        assert x is not None
        ratio = PG.tridiagonal_error(x, x_ref, cond)
        print(f"n {n} identity rows {rows}: cond {cond:.3g}, error / (cond eps) {ratio:.4f} (K = {PG.TRIDIAGONAL_K:.3f})")
        assert ratio <= PG.TRIDIAGONAL_K
        for i in rows:
            assert same_bits(x[i], b[i])  # an identity row, decoupled


@pytest.mark.parametrize("n,row", [(1, 0), (9, 4), (65, 64), (257, 0)])
def test_cyclic_reduction_flags_an_indefinite_block(L, gpu_ctx, n, row):
    D, Lo, U, b, _, _ = PG.tridiagonal_case(n)
    D = D.copy()
    D[row] = -D[row]
    D, Lo, U = [np.ascontiguousarray(a.reshape(-1, 36)) for a in (D, Lo, U)]
    x = np.full((n, 6), -7.0)
    rc = L.lib().lsa_pgo_tridiagonal_solve(gpu_ctx.h, n, L.ptr(D), L.ptr(Lo), L.ptr(U), L.ptr(np.ascontiguousarray(b)), L.ptr(x))
    assert rc == 1 and np.all(x == -7.0)
    assert gpu_ctx.pose_graph_tridiagonal_solve(D, Lo, U, b) is None
    # and the context goes on working
    D2, L2, U2, b2, x_ref, cond = PG.tridiagonal_case(n)
    assert PG.tridiagonal_error(gpu_ctx.pose_graph_tridiagonal_solve(D2, L2, U2, b2), x_ref, cond) <= PG.TRIDIAGONAL_K


def test_spmv_against_numpy_with_loop_blocks_on_the_first_and_last_rows(L, gpu_ctx):
    n = 12
    truth = [PG.circle_pose(0.3 * i, i) for i in range(n)]
    rng = np.random.default_rng(21)
    poses = np.array([PG.retract(T, 0.03 * rng.standard_normal(6)) for T in truth])
    pairs = [(i - 1, i) for i in range(1, n)] + [(0, 11), (11, 0), (0, 6), (11, 3), (4, 9), (5, 2)]
    edges = [(a, b, np.linalg.inv(truth[a]) @ truth[b], PG.random_spd(rng, 50.0)) for a, b in pairs]
    fixed = np.zeros(n, np.uint8)
    fixed[5] = 1
    for lam in (0.0, 0.5):
        H, _, _ = PG.dense_system(poses, fixed, edges, lam)
        p = rng.standard_normal((n, 6))
        q = gpu_ctx.pose_graph_spmv(poses, fixed, edges, lam, p)
        ref = (H @ p.ravel()).reshape(n, 6)  # (the fixed pose's row is the identity, its column dropped)
        assert np.abs(q - ref).max() <= 1e-12 * np.abs(ref).max()
        assert same_bits(q, L.pose_graph_spmv(poses, fixed, edges, lam, p))
        assert np.abs(H[:6, 66:]).max() > 0 and np.abs(H[66:, 18:24]).max() > 0  # blocks beyond the chain on the first and last rows


def solve_both(L, ctx, n, **kw):
    poses, fixed, edges, _ = PG.circle_graph(n)
    E = L.pose_graph_edges(edges)
    host, hres = L.pose_graph_solve_host(poses, fixed, E, **kw)
    dev, dres = ctx.pose_graph_solve(poses, fixed, E, **kw)
    return poses, fixed, E, host, hres, dev, dres


@pytest.mark.parametrize("n", [2, 3, 16, 64, 200, 257, 1000])
def test_solve_against_the_host_statement(L, gpu_ctx, n):
    poses, fixed, E, host, hres, dev, dres = solve_both(L, gpu_ctx, n)
    dpos = max(pose_diff(host[i], dev[i])[0] for i in range(n))
    drot = max(pose_diff(host[i], dev[i])[1] for i in range(n))
    print(f"n {n}: device {dres.iterations} LM / {dres.pcg_iterations} PCG iterations, termination {dres.termination}; host {hres.iterations} / {hres.pcg_iterations}, "
          f"{hres.termination}; {dpos:.2e} m {drot:.2e} rad; cost {dres.initial_cost:.5g} -> {dres.final_cost:.8g} (host {hres.final_cost:.8g})")
    assert dpos <= 1e-7 and drot <= 1e-6
    assert abs(dres.final_cost - hres.final_cost) <= 1e-9 * hres.final_cost
    assert same_bits(dres.initial_cost, hres.initial_cost) or abs(dres.initial_cost - hres.initial_cost) <= 1e-13 * hres.initial_cost
    assert dres.termination in (L.PGO_GRADIENT, L.PGO_STEP, L.PGO_COST) and dres.message
    assert dres.final_cost < 0.1 * dres.initial_cost and dres.pcg_truncated == 0
    assert max(float(np.linalg.norm(dev[i][:3, 3] - poses[i][:3, 3])) for i in range(n)) > 0.01
    assert same_bits(dev[0], poses[0])
    # twice: identical bits
    again, ares = gpu_ctx.pose_graph_solve(poses, fixed, E)
    assert same_bits(again, dev) and same_bits(ares.final_cost, dres.final_cost)
    assert (ares.iterations, ares.pcg_iterations, ares.termination) == (dres.iterations, dres.pcg_iterations, dres.termination)


def test_one_pcg_iteration_a_step_is_no_failure(L, gpu_ctx):
    """pcg_max_iter = 1: every LM step takes the truncated delta (pcg_truncated counts them); the solve ends by one of LM's own
    rules, never by LINEAR_SOLVER_FAILED, and the cost has gone down."""
    poses, fixed, E, host, hres, dev, dres = solve_both(L, gpu_ctx, 200, pcg_max_iter=1, max_iterations=12)
    for res in (hres, dres):
        assert res.termination in (L.PGO_MAX_ITERATIONS, L.PGO_STEP, L.PGO_COST, L.PGO_GRADIENT, L.PGO_LAMBDA_CEILING)
        assert res.pcg_truncated >= 1 and res.pcg_iterations == res.iterations and res.last_pcg_iterations == 1
        assert res.final_cost < res.initial_cost
    assert np.isfinite(dev).all() and dres.termination == hres.termination and dres.iterations == hres.iterations


def test_a_grossly_contradicting_loop_edge_ends_by_a_rule(L, gpu_ctx):
    poses, fixed, edges, _ = PG.circle_graph(64)
    Z = edges[-1][2].copy()
    Z[0, 3] += 1000.0  # a kilometre off
    bad = edges[:-1] + [(edges[-1][0], edges[-1][1], Z, edges[-1][3])]
    dev, res = gpu_ctx.pose_graph_solve(poses, fixed, bad, max_iterations=30)
    print("contradiction:", res)
    assert res.termination in range(6) and res.iterations <= 30 and res.message
    assert np.isfinite(dev).all() and np.isfinite(res.final_cost) and res.final_cost <= res.initial_cost


def test_refusals_write_nothing(L, gpu_ctx):
    poses, fixed, edges, _ = PG.circle_graph(16)
    P = np.ascontiguousarray(poses.reshape(-1, 16))
    p = L.PoseGraphParams()

    def refused(f, E, code=L.E_ARG):
        E = L.pose_graph_edges(E)
        out = np.full_like(P, -7.0)
        r = L.PoseGraphResultStruct()
        rc = L.lib().lsa_pgo_solve(gpu_ctx.h, L.ptr(P), 16, L.ptr(np.ascontiguousarray(f, np.uint8)), L.ptr(E), E.size, C.byref(p), L.ptr(out), C.byref(r))
        assert rc == code and np.all(out == -7.0)

    refused(np.zeros(16), edges)
    refused(fixed, [e for e in edges if 7 not in (e[0], e[1])])
    refused(fixed, edges + [(3, 16, np.eye(4), np.eye(6))])
    W = np.eye(6)
    W[1, 1] = np.inf
    refused(fixed, edges + [(3, 9, np.eye(4), W)])
    with pytest.raises(L.LsaError) as e:
        gpu_ctx.pose_graph_solve(poses, np.zeros(16), edges)
    assert e.value.code == L.E_ARG and "fixed" in str(e.value)


# ---- Slam.optimize_trajectory on the revisit of test_cpp_place_recognition.py -----------------------------------------------
MODEL, SEED, FORWARD = 16, 1000, 12


@pytest.fixture(scope="module")
def frames(L):
    return [L.synth_frame(MODEL, SEED, f) for f in range(FORWARD + 2)]


def mapped(L, frames):
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    period = frames[1][1] - frames[0][1]
    order = list(range(FORWARD)) + list(range(FORWARD - 2, -1, -1))
    for f, c in enumerate(order):
        s.add_frame(frames[c][0], frames[0][1] + f * period, f)
    return s, period, len(order)


def Rz(yaw):
    T = np.eye(4)
    T[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    return T


def loop_edge(L, s):
    P, t, cov = s.trajectory()
    q = P.shape[0] - 1
    frame, _, _, yaw = s.recognize_place(q, capacity=3, min_travelled=2.0, max_distance=0.0, exclusion_half_window=2)[0]
    reg = s.register_logged_frames(q, frame, L.LoopClosureParams(revisited_half_window=2), P[frame] @ Rz(yaw))
    assert reg.status == 0
    return (frame, q, reg.relative, L.information_from_covariance(reg.covariance))


def snapshot(L, s):
    P, t, cov = s.trajectory()
    return (s.world_transform().tobytes(), s.covariance().tobytes(), [s.map(k).tobytes() for k in (L.EDGE, L.PLANE)], P.tobytes(), t.tobytes())


def two_more(L, s, frames, period, seq):
    shots = []
    for k in range(2):
        s.add_frame(frames[1 + k][0], frames[0][1] + (seq + k) * period, seq + k)
        shots.append(snapshot(L, s))
    return shots


def test_optimize_trajectory_equals_the_host_statement_and_does_not_touch_the_frame_path(L, frames):
    s, period, n = mapped(L, frames)
    edge = loop_edge(L, s)
    P, t, cov = s.trajectory()
    before = snapshot(L, s)
    got, times, res = s.optimize_trajectory([edge])
    assert snapshot(L, s) == before and np.array_equal(times, t)
    assert s.get_param("PoseGraphSeconds") > 0
    # the same graph through the host statement
    p = L.PoseGraphParams()
    W = np.diag(1.0 / np.array(p.odometry_sigma) ** 2)
    chain = [(i - 1, i, np.linalg.inv(P[i - 1]) @ P[i], W) for i in range(1, n)]
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    host, hres = L.pose_graph_solve_host(P, fixed, chain + [edge])
    d = [pose_diff(host[i], got[i]) for i in range(n)]
    print("optimize_trajectory:", res, "against the host statement", max(a for a, _ in d), "m", max(b for _, b in d), "rad")
    assert max(a for a, _ in d) <= 1e-7 and max(b for _, b in d) <= 1e-6
    assert res.termination == hres.termination and res.final_cost <= res.initial_cost
    # apply=False: two further frames are what they are without the call
    plain, _, _ = mapped(L, frames)
    loop_edge(L, plain)
    assert two_more(L, s, frames, period, n) == two_more(L, plain, frames, period, n)
    plain.close()
    s.close()


def test_optimize_trajectory_applied_equals_set_trajectory(L, frames):
    a, period, n = mapped(L, frames)
    edge = loop_edge(L, a)
    got, times, res = a.optimize_trajectory([edge], apply=True)
    b, _, _ = mapped(L, frames)
    loop_edge(L, b)
    b.set_trajectory(got, times)
    assert snapshot(L, a) == snapshot(L, b)
    assert two_more(L, a, frames, period, n) == two_more(L, b, frames, period, n)
    # refusals, as RegisterLoggedFrames: nothing changed
    before = snapshot(L, a)
    for bad in ([(0, 99, np.eye(4), np.eye(6))], [(-1, 3, np.eye(4), np.eye(6))], [(3, 3, np.eye(4), np.eye(6))]):
        with pytest.raises(L.LsaError) as e:
            a.optimize_trajectory(bad, apply=True)
        assert e.value.code == L.E_ARG
    with pytest.raises(L.LsaError) as e:
        a.optimize_trajectory([edge], odometry_sigma=[0.0] * 6)
    assert e.value.code == L.E_ARG
    assert snapshot(L, a) == before
    off = L.Slam(0, EgoMotion=3, LoggingTimeout=0)
    for f in range(3):
        off.add_frame(frames[f][0], frames[f][1], f)
    with pytest.raises(L.LsaError) as e:
        off.optimize_trajectory([])
    assert e.value.code == L.E_STATE and "LoggingTimeout" in str(e.value)
    off.close()
    a.close()
    b.close()


def test_optimize_trajectory_with_the_logged_covariances(L, frames):
    """odometry_information = 1, the reference's rule.  Every frame of this log was localized with edges and planes in three
    dimensions, so every logged covariance is positive definite (asserted here on the log itself) and the call succeeds with
    a termination of the converged class, as mode 0 does."""
    s, period, n = mapped(L, frames)
    edge = loop_edge(L, s)
    P, t, cov = s.trajectory()
    cov = np.asarray(cov).reshape(n, 6, 6)
    assert all(np.linalg.eigvalsh(0.5 * (c + c.T)).min() > 0 for c in cov[1:])
    got, _, res = s.optimize_trajectory([edge], odometry_information=1)
    _, _, res0 = s.optimize_trajectory([edge])
    converged = (L.PGO_GRADIENT, L.PGO_STEP, L.PGO_COST)
    print("mode 1:", res)
    assert res.termination in converged and res0.termination in converged
    assert np.isfinite(got).all() and res.final_cost <= res.initial_cost
    s.close()
