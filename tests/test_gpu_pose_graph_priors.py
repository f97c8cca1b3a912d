"""Position priors in the device pose-graph solver (lidarslam_amd/csrc/lsa_pose_graph.hip) held, seam by seam, to the host
statement; Slam.run_pose_graph_optimization -- the reference's RunPoseGraphOptimization with GPS positions -- on a logged revisit."""
import ctypes as C

import numpy as np
import pytest

import pose_graph_cases as PG
import pose_graph_prior_cases as PP
from conftest import bits, pose_diff

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))


# 245 and 246 priors beside the feature graph's 11 edges: 256 and 257 values under the two-level sum, a workgroup and one more
@pytest.mark.parametrize("k", [None, 1, 245, 246, 255, 256, 257])
def test_prior_seams_equal_the_host_statement_bit_for_bit(L, gpu_ctx, k):
    poses, fixed, edges = PG.feature_graph()
    priors, O = PP.feature_priors(k)
    E, R = L.pose_graph_edges(edges), L.pose_graph_priors(priors)
    host = L.pose_graph_linearize_priors(poses, R, O)
    dev = gpu_ctx.pose_graph_linearize_priors(poses, R, O)
    assert len(host[2]) == len(priors) and np.abs(host[1]).max() > 0
    for h, d, name in zip(host, dev, ("e", "blocks", "chi2")):
        assert same_bits(h, d), (k, name, np.abs(h - d).max())
    rng = np.random.default_rng(5)
    p = rng.standard_normal((len(poses), 6))
    for lam in (0.0, 0.37):
        host = L.pose_graph_assemble(poses, fixed, E, lam, priors=R, offset=O)
        dev = gpu_ctx.pose_graph_assemble(poses, fixed, E, lam, priors=R, offset=O)
        for h, d, name in zip(host, dev, ("D", "g", "L", "U")):
            assert same_bits(h, d), (k, lam, name, np.abs(h - d).max())
        assert not same_bits(host[0], L.pose_graph_assemble(poses, fixed, E, lam)[0])  # the priors are in there
        assert same_bits(L.pose_graph_spmv(poses, fixed, E, lam, p, priors=R, offset=O), gpu_ctx.pose_graph_spmv(poses, fixed, E, lam, p, priors=R, offset=O))
    # the cost over the m + k values: the host adds them one after the other, the device in workgroups of 256 and then the
    # workgroups' sums; both are sums of m + k positive terms, each within (m + k) eps of the exact one
    _, hres = L.pose_graph_solve_host(poses, fixed, E, priors=R, offset=O, max_iterations=0)
    _, dres = gpu_ctx.pose_graph_solve(poses, fixed, E, priors=R, offset=O, max_iterations=0)
    assert hres.initial_cost > 0 and abs(dres.initial_cost - hres.initial_cost) <= 2 * (E.size + R.size) * PG.EPS * hres.initial_cost
    assert same_bits(dres.final_cost, dres.initial_cost)


def test_no_prior_gives_the_bits_of_the_solve_without_priors(L, gpu_ctx):
    poses, fixed, edges, _ = PG.circle_graph(257)
    E = L.pose_graph_edges(edges)
    plain, pres = gpu_ctx.pose_graph_solve(poses, fixed, E)
    none, nres = gpu_ctx.pose_graph_solve(poses, fixed, E, priors=[], offset=np.eye(4))
    assert same_bits(plain, none) and pres.iterations > 1
    for name in ("initial_cost", "final_cost", "largest_step", "final_lambda"):
        assert same_bits(getattr(pres, name), getattr(nres, name)), name
    assert (pres.iterations, pres.pcg_iterations, pres.termination, pres.accepted_steps) == (nres.iterations, nres.pcg_iterations, nres.termination, nres.accepted_steps)
    for lam in (0.0, 0.37):
        for h, d in zip(gpu_ctx.pose_graph_assemble(poses, fixed, E, lam), gpu_ctx.pose_graph_assemble(poses, fixed, E, lam, priors=[], offset=np.eye(4))):
            assert same_bits(h, d)


@pytest.mark.parametrize("n,s", PP.CASES + [(1000, 25)])
def test_solve_with_priors_against_the_host_statement(L, gpu_ctx, n, s):
    init, aligned, fixed, edges, priors, O, _ = PP.gps_case(n, s, tuple(PG.LOOPS[1000]) if n == 1000 else ())
    E, R = L.pose_graph_edges(edges), L.pose_graph_priors(priors)
    converged = (L.PGO_GRADIENT, L.PGO_STEP, L.PGO_COST)
    host, hres = L.pose_graph_solve_host(aligned, fixed, E, priors=R, offset=O)
    dev, dres = gpu_ctx.pose_graph_solve(aligned, fixed, E, priors=R, offset=O)
    dpos = max(pose_diff(host[i], dev[i])[0] for i in range(n))
    drot = max(pose_diff(host[i], dev[i])[1] for i in range(n))
    print(f"n {n}, {R.size} priors: device {dres.iterations} LM / {dres.pcg_iterations} PCG iterations, termination {dres.termination}; host {hres.iterations} / "
          f"{hres.pcg_iterations}, {hres.termination}; {dpos:.2e} m {drot:.2e} rad; cost {dres.initial_cost:.5g} -> {dres.final_cost:.8g} (host {hres.final_cost:.8g})")
    assert dpos <= 1e-7 and drot <= 1e-6
    assert abs(dres.final_cost - hres.final_cost) <= 1e-9 * hres.final_cost
    assert dres.termination in converged and dres.message and dres.pcg_truncated == 0 and dres.final_cost < dres.initial_cost
    if n == 1000:
        assert dres.pcg_iterations > dres.iterations  # the loop edges are PCG's
    # twice: identical bits
    again, ares = gpu_ctx.pose_graph_solve(aligned, fixed, E, priors=R, offset=O)
    assert same_bits(again, dev) and same_bits(ares.final_cost, dres.final_cost)
    assert (ares.iterations, ares.pcg_iterations, ares.termination) == (dres.iterations, dres.pcg_iterations, dres.termination)
    # from the odometry chain where it was logged, 100 m and 0.8 rad away
    far, fres = gpu_ctx.pose_graph_solve(init, fixed, E, priors=R, offset=O)
    hfar, hfres = L.pose_graph_solve_host(init, fixed, E, priors=R, offset=O)
    assert fres.termination in converged
    assert max(pose_diff(hfar[i], far[i])[0] for i in range(n)) <= 1e-7 and max(pose_diff(hfar[i], far[i])[1] for i in range(n)) <= 1e-6


def test_refusals_write_nothing(L, gpu_ctx):
    init, aligned, fixed, edges, priors, O, _ = PP.gps_case(16, 3)
    P = np.ascontiguousarray(aligned.reshape(-1, 16))
    E = L.pose_graph_edges(edges)
    Om = np.ascontiguousarray(O.reshape(16))
    p = L.PoseGraphParams()

    def refused(R, k=None):
        R = L.pose_graph_priors(R)
        out = np.full_like(P, -7.0)
        r = L.PoseGraphResultStruct()
        rc = L.lib().lsa_pgo_solve_priors(gpu_ctx.h, L.ptr(P), 16, L.ptr(fixed), L.ptr(E), E.size, L.ptr(R) if R.size else None, R.size if k is None else k, L.ptr(Om),
                                          C.byref(p), L.ptr(out), C.byref(r))
        assert rc == L.E_ARG and np.all(out == -7.0)

    refused([])
    refused(priors + [(16, np.zeros(3), np.eye(3))])
    refused(priors + [(2, np.array([np.nan, 0.0, 0.0]), np.eye(3))])
    refused(priors, k=-1)
    with pytest.raises(L.LsaError) as e:
        gpu_ctx.pose_graph_solve(aligned, fixed, E, priors=[], offset=O)
    assert e.value.code == L.E_ARG and "prior" in str(e.value)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_transforms_equal_the_host_statement_bit_for_bit(L, gpu_ctx, n):
    poses = PG.circle_graph(257)[0][:n]
    Wt = PP.world_transform()
    host = L.pose_graph_premultiply(poses, Wt)
    assert same_bits(host, gpu_ctx.pose_graph_premultiply(poses, Wt)) and np.abs(host[-1][:3, 3]).max() > 40
    back = L.pose_graph_reanchor(host)
    assert same_bits(back, gpu_ctx.pose_graph_reanchor(host)) and np.abs(back[0] - np.eye(4)).max() <= 4 * PG.EPS


# ---- Slam.run_pose_graph_optimization on the log of test_gpu_pose_graph.py: twelve frames forward and back, 23 poses -----------
MODEL, SEED, FORWARD = 16, 1000, 12
COV = np.eye(3) * 0.03**2


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


def snapshot(L, s):
    P, t, cov = s.trajectory()
    return (s.world_transform().tobytes(), s.covariance().tobytes(), [s.map(k).tobytes() for k in (L.EDGE, L.PLANE)], P.tobytes(), t.tobytes())


def two_more(L, s, frames, period, seq):
    shots = []
    for k in range(2):
        s.add_frame(frames[1 + k][0], frames[0][1] + (seq + k) * period, seq + k)
        shots.append(snapshot(L, s))
    return shots


def gps_track(P, bend=0.0):
    """the fixes of the logged poses P seen from the world Wt through the lever arm O, bent smoothly by up to `bend` metres"""
    Wt, O = PP.world_transform(), PP.lever_arm()
    n = len(P)
    g = np.array([(Wt @ P[i] @ O)[:3, 3] for i in range(n)])
    g += bend * np.sin(np.pi * np.arange(n) / (n - 1))[:, None] * np.array([0.0, 0.8, 0.6])
    return g, np.repeat(COV[None], n, 0), Wt, O


def test_exact_gps_gives_back_the_logged_trajectory_in_the_gps_frame(L, frames):
    s, period, n = mapped(L, frames)
    P, t, _ = s.trajectory()
    g, cov, Wt, O = gps_track(P)
    before = snapshot(L, s)
    got, times, cal, res, matches = s.run_pose_graph_optimization(t, g, cov, gps_to_sensor=np.linalg.inv(O), apply=False)
    print("exact GPS:", res)
    assert snapshot(L, s) == before and np.array_equal(times, t) and list(matches) == list(range(n))
    assert s.get_param("PoseGraphSeconds") > 0
    assert res.final_cost <= 1e-12 * res.initial_cost + 1e-18
    d = [pose_diff(np.linalg.inv(P[0]) @ P[i], got[i]) for i in range(n)]
    assert max(a for a, _ in d) <= 1e-7 and max(b for _, b in d) <= 1e-6
    dpos, drot = pose_diff(Wt @ P[0], cal)
    print(f"calibration: {dpos:.2e} m {drot:.2e} rad")
    assert dpos <= 1e-7 and drot <= 1e-6
    # apply=False: two further frames are what they are without the call
    plain, _, _ = mapped(L, frames)
    assert two_more(L, s, frames, period, n) == two_more(L, plain, frames, period, n)
    plain.close()
    s.close()


def test_bent_gps_equals_the_host_statement_and_applied_equals_set_trajectory(L, frames):
    a, period, n = mapped(L, frames)
    P, t, lcov = a.trajectory()
    g, cov, Wt, O = gps_track(P, 0.2)
    got, times, cal, res, matches = a.run_pose_graph_optimization(t, g, cov, gps_to_sensor=np.linalg.inv(O), apply=True)
    # the same graph through the host statement from the same aligned start
    lcov = np.asarray(lcov).reshape(n, 6, 6)
    chain = [(i - 1, i, np.linalg.inv(P[i - 1]) @ P[i], L.information_from_covariance(lcov[i])) for i in range(1, n)]
    priors = [(i, g[i], L.information_from_covariance3(cov[i])) for i in range(n)]
    W = L.trajectory_alignment([(P[i] @ O)[:3, 3] for i in range(n)], g)
    start = L.pose_graph_premultiply(P, W)
    host, hres = L.pose_graph_solve_host(start, np.zeros(n, np.uint8), chain, priors=priors, offset=O, odometry_information=1)
    back = L.pose_graph_reanchor(host)
    d = [pose_diff(back[i], got[i]) for i in range(n)]
    print("bent GPS:", res, "against the host statement", max(x for x, _ in d), "m", max(y for _, y in d), "rad")
    assert max(x for x, _ in d) <= 1e-7 and max(y for _, y in d) <= 1e-6
    assert res.termination == hres.termination and res.final_cost < res.initial_cost
    assert pose_diff(host[0], cal)[0] <= 1e-7 and pose_diff(host[0], cal)[1] <= 1e-6
    assert max(float(np.linalg.norm(got[i][:3, 3] - (np.linalg.inv(P[0]) @ P[i])[:3, 3])) for i in range(n)) > 0.01  # the bend is in there
    # applied: what set_trajectory makes of the same poses
    b, _, _ = mapped(L, frames)
    b.set_trajectory(got, times)
    assert snapshot(L, a) == snapshot(L, b)
    assert two_more(L, a, frames, period, n) == two_more(L, b, frames, period, n)
    a.close()
    b.close()


def test_refusals_change_nothing(L, frames):
    s, period, n = mapped(L, frames)
    P, t, _ = s.trajectory()
    g, cov, Wt, O = gps_track(P)
    cal = np.linalg.inv(O)
    before = snapshot(L, s)
    singular = cov.copy()
    singular[5] = np.diag([1e-3, 1e-3, 0.0])
    span = t[-1] - t[0]
    for args, code, word in (((t[:1], g[:1], cov[:1]), L.E_ARG, "at least 2"), ((t + 10 * span, g, cov), L.E_ARG, "time offset"), ((t, g, singular), L.E_ARG, "fix 5")):
        with pytest.raises(L.LsaError) as e:
            s.run_pose_graph_optimization(*args, gps_to_sensor=cal, apply=True)
        assert e.value.code == code and word in str(e.value), str(e.value)
    assert snapshot(L, s) == before
    # a time offset brings shifted fixes back
    _, _, _, res, matches = s.run_pose_graph_optimization(t + 10 * span, g, cov, gps_to_sensor=cal, apply=False, time_offset=10 * span)
    assert list(matches) == list(range(n)) and snapshot(L, s) == before
    s.close()
    off, _, _ = mapped(L, frames, LoggingTimeout=0)
    with pytest.raises(L.LsaError) as e:
        off.run_pose_graph_optimization(t, g, cov, gps_to_sensor=cal)
    assert e.value.code == L.E_STATE and "LoggingTimeout" in str(e.value)
    off.close()
