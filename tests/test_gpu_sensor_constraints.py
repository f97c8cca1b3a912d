"""Wheel odometer and IMU gravity terms in the localization solve, on the device: lsa_accumulate and the one-launch
solve (k_lm_solve) with the terms against the host-driven loop and the host evaluation of the terms, an optimum
worked out here by a damped Newton iteration, and the pipeline (in-line and linked ICP iterations) fed with
measurement streams built from the generator's ground truth."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPEED, YAW_AMP, OMEGA, SWEEP = 5.0, 3.0 * math.pi / 180.0, 2.0 * math.pi / 10.0, 0.1  # lsa_synth.cpp


def perturbed(dx=0.45, yaw=0.01):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    T[:3, 3] = [dx, 0.02, 0.0]
    return T


@pytest.fixture(scope="module")
def kps(O, L):
    out = {}
    for model in (16, 64):
        ex = O.Extractor()
        per = []
        for f in range(2):
            pts, _ = L.synth_frame(model, 1000, f)
            ex.compute(pts)
            per.append([ex.keypoints(k) for k in range(3)])
        out[model] = per
    return out


def setup_residuals(ctx, L, kps, model):
    """as tests/test_gpu_match.py::setup_residuals: ego-motion matches of two scans under a perturbed pose"""
    prev, cur = kps[model]
    mp = L.MatchParams.ego_motion(saturation_distance=5.0)
    for k in (0, 1):
        ctx.set_keypoints(L.SET_WORKING, k, cur[k])
        ctx.set_target(k, prev[k])
        ctx.match(k, L.SET_WORKING, mp, perturbed())
    ctx.set_keypoints(L.SET_WORKING, 2, cur[2][:0])
    ctx.match(2, L.SET_WORKING, mp, perturbed())


def terms_for(L, which):
    g_cur = np.array([0.0, math.sin(0.03), math.cos(0.03)])
    return {
        "wheel": L.SensorTerms(wheel_weight=40.0, d=0.52),
        "gravity": L.SensorTerms(gravity_weight=500.0, g_ref=(0.0, 0.0, 1.0), g_cur=g_cur),
        "both": L.SensorTerms(wheel_weight=40.0, d=0.52, gravity_weight=500.0, g_ref=(0.0, 0.0, 1.0), g_cur=g_cur),
    }[which]


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("model", [16, 64])
def test_accumulate_adds_exactly_the_terms(gpu_ctx, L, kps, model):
    setup_residuals(gpu_ctx, L, kps, model)
    w_ref = np.array([0.45, 0.01, -0.02, 0.001, -0.002, 0.012])
    before = gpu_ctx.accumulate(7, w_ref)
    for which in ("wheel", "gravity", "both"):
        t = terms_for(L, which)
        for w in (np.array([0.45, 0.01, -0.02, 0.001, -0.002, 0.012]), np.array([0.3, 0.2, 0.1, 0.2, -0.3, 1.1]), np.zeros(6)):
            gpu_ctx.set_sensor_terms(None)
            c0, g0, H0, n0 = gpu_ctx.accumulate(7, w)
            ct, gt, Ht, nt = L.sums_to_normal_equations(L.sensor_terms_eval(t, w))
            gpu_ctx.set_sensor_terms(t)
            c1, g1, H1, n1 = gpu_ctx.accumulate(7, w)
            cc, _, _, _ = gpu_ctx.accumulate(7, w, jac=False)
            gpu_ctx.set_sensor_terms(None)
            assert n1 == n0 and nt == 0  # the match count is the LiDAR's alone
            assert abs(c1 - (c0 + ct)) <= 1e-12 * (c0 + ct) and cc == c1
            assert rel(g1, g0 + gt) <= 1e-12 and rel(H1, H0 + Ht) <= 1e-12 and np.array_equal(H1, H1.T)
    # cleared: bit for bit what it was before any terms were set
    after = gpu_ctx.accumulate(7, w_ref)
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2]) and after[3] == before[3]


@pytest.mark.parametrize("two_d", [False, True])
@pytest.mark.parametrize("model", [16, 64])
def test_one_launch_solve_with_terms_equals_the_host_driven_loop(gpu_ctx, L, kps, model, two_d):
    setup_residuals(gpu_ctx, L, kps, model)
    w0 = np.array([0.45, 0.02, 0.0, 0.0, 0.0, 0.01])
    fallbacks = gpu_ctx.solve_device_fallbacks()  # (counted over the context's life: other tests provoke some on purpose)
    gpu_ctx.set_sensor_terms(None)
    base = gpu_ctx.solve_device(7, w0, max_iter=15, two_d=two_d)
    for which in ("wheel", "gravity", "both"):
        gpu_ctx.set_sensor_terms(terms_for(L, which))
        r = gpu_ctx.solve_device(7, w0, max_iter=15, two_d=two_d)
        pose, summ, costs = gpu_ctx.solve(7, perturbed(0.45, 0.01), max_iter=15, two_d=two_d)
        r2 = gpu_ctx.solve_device(7, w0, max_iter=15, two_d=two_d)
        gpu_ctx.set_sensor_terms(None)
        assert (r.num_successful_steps, r.num_unsuccessful_steps, r.num_iterations, r.num_evaluations) == tuple(summ)
        x = np.array(r.pose)
        cx, sx, cy, sy, cz, sz = np.cos(x[3]), np.sin(x[3]), np.cos(x[4]), np.sin(x[4]), np.cos(x[5]), np.sin(x[5])
        R = np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz], [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz], [-sy, sx * cy, cx * cy]])
        assert np.abs(R - pose[:3, :3]).max() < 1e-9 and np.abs(x[:3] - pose[:3, 3]).max() < 1e-9
        assert abs(r.final_cost - costs[1]) <= 1e-10 * costs[1] and abs(r.initial_cost - costs[0]) <= 1e-10 * costs[0]
        assert list(r2.pose) == list(r.pose) and r2.final_cost == r.final_cost and list(r2.H) == list(r.H)
        assert r.num_matches == base.num_matches and not r.skipped
        if which != "wheel":
            assert list(r.pose) != list(base.pose)
        if two_d:
            assert r.pose[2] == w0[2] and r.pose[3] == w0[3] and r.pose[4] == w0[4]  # Z, rX, rY held
    again = gpu_ctx.solve_device(7, w0, max_iter=15, two_d=two_d)
    assert list(again.pose) == list(base.pose) and again.final_cost == base.final_cost and list(again.H) == list(base.H)
    assert gpu_ctx.solve_device_fallbacks() == fallbacks


def np_terms(t, w):
    """the two terms at w in numpy (cost, g, H), written from their definitions"""
    g, H, cost = np.zeros(6), np.zeros((6, 6)), 0.0
    if t.wheel:
        d = w[:3] - np.array(t.p)
        n = np.linalg.norm(d)
        r = (n if n * n >= 1e-6 else 0.0) - t.d
        cost += 0.5 * t.wheel_weight * r * r
        if n * n >= 1e-6:
            J = np.zeros(6)
            J[:3] = d / n
            g += t.wheel_weight * J * r
            H += t.wheel_weight * np.outer(J, J)
    if t.gravity:
        cx, sx, cy, sy, cz, sz = np.cos(w[3]), np.sin(w[3]), np.cos(w[4]), np.sin(w[4]), np.cos(w[5]), np.sin(w[5])
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        dRx = np.array([[0, 0, 0], [0, -sx, -cx], [0, cx, -sx]])
        dRy = np.array([[-sy, 0, cy], [0, 0, 0], [-cy, 0, -sy]])
        dRz = np.array([[-sz, -cz, 0], [cz, -sz, 0], [0, 0, 0]])
        gc = np.array(t.g_cur)
        r = Rz @ Ry @ Rx @ gc - np.array(t.g_ref)
        J = np.zeros((3, 6))
        J[:, 3], J[:, 4], J[:, 5] = Rz @ Ry @ dRx @ gc, Rz @ dRy @ Rx @ gc, dRz @ Ry @ Rx @ gc
        cost += 0.5 * t.gravity_weight * r @ r
        g += t.gravity_weight * J.T @ r
        H += t.gravity_weight * J.T @ J
    return cost, g, H


@pytest.mark.parametrize("model", [16, 64])
def test_the_solve_finds_the_optimum_of_an_independent_newton_iteration(gpu_ctx, L, kps, model):
    setup_residuals(gpu_ctx, L, kps, model)
    t = terms_for(L, "both")
    w0 = np.array([0.45, 0.02, 0.0, 0.0, 0.0, 0.01])
    gpu_ctx.set_sensor_terms(t)
    r = gpu_ctx.solve_device(7, w0, max_iter=50)
    gpu_ctx.set_sensor_terms(None)

    def f(w):
        c, g, H, _ = gpu_ctx.accumulate(7, w)  # the LiDAR terms alone
        ct, gt, Ht = np_terms(t, w)
        return c + ct, g + gt, H + Ht

    w, lam = w0.copy(), 1e-3
    c, g, H = f(w)
    for _ in range(200):
        step = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        cn, gn, Hn = f(w + step)
        if cn < c:
            w, c, g, H, lam = w + step, cn, gn, Hn, lam / 10
            if np.abs(step).max() < 1e-12:
                break
        else:
            lam *= 10
    dpos, drot = float(np.abs(np.array(r.pose[:3]) - w[:3]).max()), float(np.abs(np.array(r.pose[3:]) - w[3:]).max())
    print(f"model {model}: solve vs Newton optimum {dpos:.3e} m {drot:.3e} rad, |g| at the optimum {np.abs(g).max():.3e}")
    # measured on the first run: 5.7e-6 m / 4.0e-6 rad (VLP-16), 2.4e-6 m / 1.4e-7 rad (HDL-64) -- the solve stops at
    # Ceres' function tolerance (relative cost change 1e-6), the Newton iteration here at a step of 1e-12
    assert dpos < 2e-5 and drot < 2e-5


# ---- pipeline ----------------------------------------------------------------------------------------------------------
def arc_length(t):
    # |d/dt (x, y)| = sqrt(5^2 + (5 A sin(w t))^2): integrated by Simpson's rule on a fine grid
    n = max(2, int(math.ceil(t / 1e-3)) * 2)
    s = np.linspace(0.0, t, n + 1)
    v = np.sqrt(SPEED ** 2 + (SPEED * YAW_AMP * np.sin(OMEGA * s)) ** 2)
    h = t / n
    return float(h / 3 * (v[0] + v[-1] + 4 * v[1:-1:2].sum() + 2 * v[2:-1:2].sum()))


def run(L, model, nframes, params, feed=None, per_frame=None):
    """a sequence; `feed` lists (time, kind, value) measurements, handed over as a live system would: those up to
    50 ms past a frame's stamp before the frame"""
    s = L.Slam(0, **params)
    pending = sorted(feed or [], key=lambda m: m[0])
    poses, terms = [], []
    for f in range(nframes):
        pts, stamp = L.synth_frame(model, 1000, f)
        while pending and pending[0][0] <= stamp * 1e-6 + 0.05:
            t, kind, value = pending.pop(0)
            if kind == "wheel":
                s.add_wheel_odom(t, value)
            else:
                s.add_gravity(t, value)
        s.add_frame(pts, stamp, f)
        poses.append(s.world_transform())
        terms.append(s.sensor_terms().as_tuple())
        if per_frame:
            per_frame(s, f)
    out = {"poses": np.array(poses), "terms": terms, "cov": s.covariance().copy(), "fallbacks": s.get_param("DeviceSolveFallbacks")}
    s.close()
    return out


def feed_wheel(bias=0.0):
    """the odometer at 100 Hz: arc length of the generator's path (5 m/s), scaled by 1 + bias"""
    return [(k * 0.01, "wheel", (1.0 + bias) * arc_length(k * 0.01)) for k in range(400)]


def feed_imu(tilt_deg=0.0):
    """the IMU at 100 Hz: gravity along +z, tilted by `tilt_deg` in roll after the first second"""
    a = math.radians(tilt_deg)
    return [(k * 0.01, "imu", [0.0, 9.81 * math.sin(a if k >= 100 else 0.0), 9.81 * math.cos(a if k >= 100 else 0.0)]) for k in range(400)]


def feed_both():
    return feed_wheel() + feed_imu()


@pytest.mark.parametrize("model,nframes", [(16, 30), (64, 10)])
def test_pipeline_forms_agree_with_the_terms_on(L, model, nframes):
    params = dict(EgoMotion=3, WheelOdomWeight=20.0, GravityWeight=50.0)
    runs = {name: run(L, model, nframes, dict(params, **extra), feed_both()) for name, extra in
            (("inline", {"DeviceLM": 0}), ("links", {}))}
    for name, r in runs.items():
        assert r["fallbacks"] == 0, name
        assert np.abs(r["poses"][:, :3, 3] - runs["links"]["poses"][:, :3, 3]).max() < 1e-9, name
        assert np.abs(r["poses"][:, :3, :3] - runs["links"]["poses"][:, :3, :3]).max() < 1e-9, name
        assert r["terms"] == runs["links"]["terms"], name
    terms = runs["links"]["terms"]
    # frame 0 sets the odometer's baseline; from frame 1 on both terms are in, d = the arc length since frame 0
    assert terms[0][0] == 0 and terms[0][6] == 1
    for f in range(1, nframes):
        wheel, ww, p0, p1, p2, d, grav, gw, *g = terms[f]
        assert (wheel, ww, p0, p1, p2, grav, gw) == (1, 20.0, 0.0, 0.0, 0.0, 1, 50.0)
        assert abs(d - (arc_length(SWEEP * (f + 1)) - arc_length(SWEEP))) < 1e-9
        assert np.abs(np.array(g) - [0, 0, 1, 0, 0, 1]).max() < 1e-12
    # the covariance comes from the same problem
    plain = run(L, model, nframes, dict(EgoMotion=3))
    assert not np.array_equal(plain["cov"], runs["links"]["cov"])


def test_zero_weights_are_bit_identical_to_no_sensor_calls(L):
    plain = run(L, 16, 30, dict(EgoMotion=3))
    fed = run(L, 16, 30, dict(EgoMotion=3), feed_both())
    assert np.array_equal(plain["poses"], fed["poses"]) and np.array_equal(plain["cov"], fed["cov"])
    assert all(t == tuple([0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]) for t in fed["terms"])


def test_a_biased_odometer_pulls_the_trajectory_along(L):
    dist = [float(np.linalg.norm(run(L, 16, 30, dict(EgoMotion=3, WheelOdomWeight=w), feed_wheel(0.05))["poses"][-1][:3, 3])) for w in (0.0, 50.0, 5000.0)]
    print("final |t| over the odometer weights 0 / 50 / 5000:", dist)
    assert dist[0] < dist[1] < dist[2]


def test_a_tilted_imu_turns_the_roll_toward_the_tilt(L):
    def roll(T):
        return math.atan2(T[2, 1], T[2, 2])
    rolls = [roll(run(L, 16, 30, dict(EgoMotion=3, GravityWeight=w), feed_imu(2.0))["poses"][-1]) for w in (0.0, 100.0, 10000.0)]
    print("final roll [deg] over the gravity weights 0 / 100 / 10000:", [math.degrees(r) for r in rolls])
    # the LiDAR alone ends at -0.83 degrees of roll on this sequence; the IMU's +2 degrees pull it up as the weight grows
    assert rolls[0] < rolls[1] < rolls[2] <= math.radians(2.0) + 1e-3


def test_terms_stay_while_no_manager_is_usable_and_clear_ends_them(L):
    def per_frame(s, f):
        if f == 5:
            s.set_param("WheelOdomWeight", 0.0)  # quirk 1: the last terms stay in the problem
        if f == 9:
            s.clear_sensor_measurements()
    r = run(L, 16, 12, dict(EgoMotion=3, WheelOdomWeight=20.0), feed_wheel(), per_frame)
    t = r["terms"]
    assert t[1][0] == 1 and t[5][0] == 1 and t[6] == t[5] and t[9] == t[5]
    assert t[10][0] == 0 and t[11][0] == 0
