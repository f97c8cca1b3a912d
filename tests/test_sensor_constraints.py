"""Wheel odometer and IMU gravity constraints, without a device: the measurement managers (lsa_sensors_*) against a
plain-Python restatement of SensorConstraints.cxx written here, bit for bit, and the residual arithmetic shared with
the solve kernel (lsa_sensor_terms_eval) against mpmath at 30 digits."""
import math

import mpmath as mp
import numpy as np
import pytest

# Utils::Deg2Rad(5.f): 5 / 180 * pi in double, returned as float
DELTA = float(np.float32(5.0 / 180.0 * math.pi))
N_PHI, N_THETA = math.ceil(2 * math.pi / DELTA), math.ceil(math.pi / DELTA)


def norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def normalized(v):
    sq = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    if sq > 0:
        n = math.sqrt(sq)
        return [v[0] / n, v[1] / n, v[2] / n]
    return list(v)


class Managers:
    """SensorConstraints.h / .cxx (absolute wheel mode, IMU gravity) and Slam::ComputeSensorConstraints' call rule,
    with the out-of-bounds reads of the reference defined: index -1 -> 0, one measurement -> its value, two at the
    same time -> the earlier one, the last histogram bin for phi / theta = pi."""

    def __init__(self):
        self.wheel, self.imu = [], []
        self.ww = self.gw = self.offset = 0.0
        self.wprev = self.iprev = -1
        self.prev_dist = 0.0
        self.gref = [0.0, 0.0, 0.0]
        self.terms = self.empty()

    @staticmethod
    def empty():
        return [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]

    def clear(self):
        self.wheel, self.imu = [], []
        self.wprev = self.iprev = -1
        self.offset = 0.0
        self.terms = self.empty()

    def usable(self):
        return (self.ww > 1e-6 and bool(self.wheel)), (self.gw > 1e-6 and bool(self.imu))

    def compute(self, t):
        if any(self.usable()):
            self._wheel(t)
            self._gravity(t)
        return tuple(self.terms)

    @staticmethod
    def _index(m, prev, t):
        idx = prev
        while idx + 1 < len(m) and m[idx + 1][0] < t:
            idx += 1
        idx = max(idx, 0)
        if idx + 1 >= len(m):
            return idx, 0.0, idx
        dt = m[idx + 1][0] - m[idx][0]
        return idx, ((t - m[idx][0]) / dt if dt > 0 else 0.0), idx + 1

    def _wheel(self, t):
        self.terms[0:6] = [0, 0.0, 0.0, 0.0, 0.0, 0.0]
        if not self.usable()[0]:
            return
        t -= self.offset
        if t < self.wheel[0][0] or t > self.wheel[-1][0]:
            return
        if self.wprev >= 0 and self.wheel[self.wprev][0] > t:
            self.wprev = -1
        idx, rt, nxt = self._index(self.wheel, self.wprev, t)
        dist = (1 - rt) * self.wheel[idx][1] + rt * self.wheel[nxt][1]
        if self.wprev == -1:
            self.wprev, self.prev_dist = idx, dist
            return
        self.terms[0:6] = [1, self.ww, 0.0, 0.0, 0.0, dist - self.prev_dist]
        self.wprev = idx

    def _gravity_ref(self):
        count = [0] * (N_PHI * N_THETA)
        bins = []
        for _, acc in self.imu:
            d = normalized(acc)
            ip = min(int((math.atan2(d[1], d[0]) + math.pi) / DELTA), N_PHI - 1)
            it = min(int(math.acos(min(max(d[2], -1.0), 1.0)) / DELTA), N_THETA - 1)
            bins.append(ip * N_THETA + it)
            count[bins[-1]] += 1
        best = 0
        for k in range(len(count)):
            if count[k] > count[best]:
                best = k
        s = [0.0, 0.0, 0.0]
        for b, (_, acc) in zip(bins, self.imu):
            if b == best:
                d = normalized(acc)
                s = [s[0] + d[0], s[1] + d[1], s[2] + d[2]]
        self.gref = normalized(s)

    def _gravity(self, t):
        self.terms[6:14] = [0, 0.0] + [0.0] * 6
        if not self.usable()[1]:
            return
        t -= self.offset
        if t < self.imu[0][0] or t > self.imu[-1][0]:
            return
        if norm3(self.gref) < 1e-6:
            self._gravity_ref()
        if self.iprev >= 0 and self.imu[self.iprev][0] > t:
            self.iprev = -1
        idx, rt, nxt = self._index(self.imu, self.iprev, t)
        a, b = normalized(self.imu[idx][1]), normalized(self.imu[nxt][1])
        g = [(1 - rt) * a[i] + rt * b[i] for i in range(3)]
        n = norm3(g)
        if not n > 1e-6:
            return
        self.terms[6:14] = [1, self.gw] + list(self.gref) + [g[0] / n, g[1] / n, g[2] / n]
        self.iprev = idx


class Pair:
    """the product's managers and the restatement, driven together"""

    def __init__(self, L):
        self.c, self.p = L.Sensors(), Managers()

    def wheel(self, t, d):
        self.c.add_wheel_odom(t, d)
        self.p.wheel.append((t, d))

    def imu(self, t, acc):
        self.c.add_gravity(t, acc)
        self.p.imu.append((t, [float(v) for v in acc]))

    def weights(self, ww, gw):
        self.c.set_weights(ww, gw)
        self.p.ww, self.p.gw = ww, gw

    def offset(self, o):
        self.c.set_time_offset(o)
        self.p.offset = o

    def clear(self):
        self.c.clear()
        self.p.clear()

    def compute(self, t):
        got, want = self.c.compute(t).as_tuple(), self.p.compute(t)
        assert [bits(v) for v in got] == [bits(v) for v in want], (t, got, want)
        g, have = self.c.gravity_ref()
        assert [bits(v) for v in g] == [bits(v) for v in self.p.gref]
        return got


def bits(v):
    return np.float64(v).view(np.uint64).item() if isinstance(v, float) else v


def test_histogram_size_follows_the_float_bin_width():
    # Deg2Rad<float> rounds 5 degrees down: 2 pi / delta is 72.000002..., so there are 73 phi bins and 37 theta bins,
    # and phi = pi / theta = pi fall into bins 72 / 36 -- the last ones
    assert DELTA < 5.0 / 180.0 * math.pi and (N_PHI, N_THETA) == (73, 37)
    assert int((math.pi + math.pi) / DELTA) == N_PHI - 1 and int(math.pi / DELTA) == N_THETA - 1


@pytest.mark.parametrize("seed", range(12))
def test_managers_equal_the_restatement_on_random_streams(L, seed):
    rng = np.random.default_rng(seed)
    s = Pair(L)
    s.weights(float(rng.choice([0.0, 0.5, 2.0])), float(rng.choice([0.0, 1.0, 10.0])))
    t0 = float(rng.uniform(0, 100))
    n = int(rng.integers(1, 60))
    tw = t0 + np.cumsum(rng.uniform(0.005, 0.2, n))
    ti = t0 + np.cumsum(rng.uniform(0.005, 0.05, 2 * n))
    if seed % 4 == 1:
        ti[3:5] = ti[3]  # two IMU measurements at the same time
    dist = np.cumsum(rng.uniform(0, 1, n))
    tilt = rng.normal(0, 0.05, (2 * n, 3))
    for t, d in zip(tw, dist):
        s.wheel(float(t), float(d))
    for t, e in zip(ti, tilt):
        s.imu(float(t), [float(e[0]), float(e[1]), float(9.81 + e[2])])
    lo, hi = min(tw[0], ti[0]) - 0.3, max(tw[-1], ti[-1]) + 0.3
    times = list(rng.uniform(lo, hi, 40))
    times.sort()
    times[5:5] = [float(tw[0]), float(ti[0]), float(tw[-1]), float(tw[min(3, n - 1)])]  # exactly on measurements
    times[20:20] = [float(t) - 1.0 for t in times[10:14]]  # the timeline goes back
    for k, t in enumerate(times):
        if k == 25:
            s.offset(float(rng.uniform(-0.1, 0.1)))
        if k == 30:
            s.weights(float(rng.choice([0.0, 1.5])), float(rng.choice([0.0, 3.0])))  # quirk 1 when both go to 0
        s.compute(float(t))


def test_first_frame_baseline_and_distance_from_it(L):
    s = Pair(L)
    s.weights(1.0, 0.0)
    for k in range(11):
        s.wheel(10.0 + k, 2.0 * k)
    assert s.compute(9.0)[0] == 0  # before the first measurement: no constraint, no baseline
    assert s.compute(10.0)[0] == 0  # the first usable frame (the LiDAR time is the first measurement's): baseline 0
    t = s.compute(12.5)
    assert t[0] == 1 and t[1] == 1.0 and t[5] == 5.0  # from the first frame, never updated
    t = s.compute(15.0)
    assert t[5] == 10.0
    assert s.compute(30.0)[0] == 0  # after the last measurement
    t = s.compute(11.0)  # the timeline went back: a new baseline, no constraint
    assert t[0] == 0
    assert s.compute(13.0)[5] == 4.0


def test_single_measurement_and_time_offset(L):
    s = Pair(L)
    s.weights(1.0, 1.0)
    s.wheel(5.0, 1.0)
    s.imu(5.0, [0.0, 0.0, 9.8])
    t = s.compute(5.0)  # one measurement each, at the LiDAR time: its value (the reference reads index -1 and 1)
    assert t[0] == 0 and t[6] == 1 and list(t[8:14]) == [0.0, 0.0, 1.0, 0.0, 0.0, 1.0]
    s.offset(0.5)
    assert s.compute(5.5)[6] == 1 and s.compute(5.0)[6] == 0  # 5.0 - 0.5 is outside the measurements


def test_clear_keeps_the_gravity_reference_and_zeroes_the_offset(L):
    s = Pair(L)
    s.weights(2.0, 3.0)
    for k in range(5):
        s.wheel(float(k), float(k))
        s.imu(float(k), [0.1, 0.0, 1.0])
    s.offset(0.25)
    s.compute(1.25)
    t = s.compute(2.25)
    assert t[0] == 1 and t[6] == 1
    gref = s.c.gravity_ref()[0].copy()
    s.clear()
    assert s.c.compute(2.0).as_tuple() == tuple(Managers.empty())  # residuals gone, and nothing usable: nothing computed
    assert np.array_equal(s.c.gravity_ref()[0], gref)  # kept
    s.p.clear()
    for k in range(5):
        s.wheel(float(k), 10.0 + k)
        s.imu(float(k), [0.0, 0.5, 1.0])  # another direction: the kept reference is not recomputed
    t = s.compute(2.0)  # offset 0 now; the odometer starts from a new baseline
    assert t[0] == 0 and t[6] == 1 and list(t[8:11]) == list(gref)


def test_stale_terms_while_neither_manager_is_usable(L):
    s = Pair(L)
    s.weights(1.0, 2.0)
    for k in range(10):
        s.wheel(float(k), 3.0 * k)
        s.imu(float(k), [0.0, 0.0, 1.0])
    s.compute(1.0)
    before = s.compute(4.0)
    s.weights(0.0, 0.0)  # the weights go to 0 mid-sequence: ComputeSensorConstraints is not called ...
    assert s.compute(6.0) == before  # ... and the last terms stay, with their old weights
    s.weights(0.0, 1.0)  # one usable again: both recompute, the odometer's term is reset
    t = s.compute(7.0)
    assert t[0] == 0 and t[6] == 1 and t[7] == 1.0


def test_histogram_edges_and_ties(L):
    s = Pair(L)
    s.weights(0.0, 1.0)
    # phi = pi (y = +0, x < 0): bin (72, 18); theta = pi (straight down): bin (36, 36); a zero vector (atan2(0, 0) = 0,
    # acos(0)): bin (36, 18), with +x.  Three bins of two each: the first fullest in (phi, theta) order wins, and the
    # zero vector adds nothing to the mean
    for k, acc in enumerate([[-1.0, 0.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 0.0, -3.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]):
        s.imu(float(k), acc)
    s.compute(2.5)
    g, have = s.c.gravity_ref()
    assert have and list(g) == [1.0, 0.0, 0.0]
    # zero accelerations around the LiDAR time: no constraint (norm <= 1e-6)
    z = Pair(L)
    z.weights(0.0, 1.0)
    z.imu(0.0, [0.0, 0.0, 1.0])
    z.imu(1.0, [0.0, 0.0, 0.0])
    z.imu(2.0, [0.0, 0.0, 0.0])
    assert z.compute(1.5)[6] == 0
    assert z.compute(0.5)[6] == 1


# ---- the residual arithmetic (lsa_sensor_terms.h) against mpmath -----------------------------------------------------
mp.mp.dps = 30


def mp_terms(terms, w):
    """29 sums of the two residuals at w, in mpmath (the same definitions: r = |t - p| - d with the 1e-6 guard,
    r = R(rx, ry, rz) gc - gr, R = Rz Ry Rx)"""
    out = [mp.mpf(0)] * 29
    W = [mp.mpf(v) for v in w]
    J = [[mp.mpf(0)] * 6 for _ in range(4)]
    r = [mp.mpf(0)] * 4
    wt = [mp.mpf(0)] * 4
    if terms.wheel:
        d = [W[i] - mp.mpf(terms.p[i]) for i in range(3)]
        sq = d[0] ** 2 + d[1] ** 2 + d[2] ** 2
        live = sq >= mp.mpf(1e-6)
        n = mp.sqrt(sq) if live else mp.mpf(0)
        r[0] = n - mp.mpf(terms.d)
        wt[0] = mp.mpf(terms.wheel_weight)
        if live:
            for i in range(3):
                J[0][i] = d[i] / n
    if terms.gravity:
        cx, sx, cy, sy, cz, sz = mp.cos(W[3]), mp.sin(W[3]), mp.cos(W[4]), mp.sin(W[4]), mp.cos(W[5]), mp.sin(W[5])
        Rx = mp.matrix([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        Ry = mp.matrix([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        Rz = mp.matrix([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        dRx = mp.matrix([[0, 0, 0], [0, -sx, -cx], [0, cx, -sx]])
        dRy = mp.matrix([[-sy, 0, cy], [0, 0, 0], [-cy, 0, -sy]])
        dRz = mp.matrix([[-sz, -cz, 0], [cz, -sz, 0], [0, 0, 0]])
        gc = mp.matrix([mp.mpf(v) for v in terms.g_cur])
        R = Rz * Ry * Rx
        res = R * gc
        cols = [Rz * Ry * dRx * gc, Rz * dRy * Rx * gc, dRz * Ry * Rx * gc]
        for i in range(3):
            r[1 + i] = res[i] - mp.mpf(terms.g_ref[i])
            wt[1 + i] = mp.mpf(terms.gravity_weight)
            for k in range(3):
                J[1 + i][3 + k] = cols[k][i]
    for i in range(4):
        out[0] += wt[i] * r[i] ** 2 / 2
    h = 7
    for a in range(6):
        out[1 + a] = sum(wt[i] * J[i][a] * r[i] for i in range(4))
        for b in range(a, 6):
            out[h] = sum(wt[i] * J[i][a] * J[i][b] for i in range(4))
            h += 1
    return out


def check_terms(L, terms, w, scale):
    got = L.sensor_terms_eval(terms, w)
    want = mp_terms(terms, w)
    for k in range(29):
        err = abs(mp.mpf(got[k]) - want[k])
        assert err <= mp.mpf(1e-13) * max(abs(want[k]), mp.mpf(scale)), (k, got[k], want[k], terms.as_tuple(), list(w))
    assert got[28] == 0.0  # the LiDAR match count is not touched
    return got


@pytest.mark.parametrize("seed", range(8))
def test_terms_eval_equals_mpmath(L, seed):
    rng = np.random.default_rng(100 + seed)
    for _ in range(25):
        w = np.concatenate([rng.normal(0, 20, 3), rng.uniform(-math.pi, math.pi, 3) * (4.0 if seed % 2 else 1.0)])  # large angles too
        p = rng.normal(0, 5, 3)
        d = float(rng.uniform(0, 60))
        g_cur = normalized(list(rng.normal(0, 1, 3)))
        g_ref = normalized(list(rng.normal(0, 1, 3)))
        ww, gw = float(rng.uniform(0.01, 10)), float(rng.uniform(0.01, 10))
        t = L.SensorTerms(wheel_weight=ww, p=p, d=d, gravity_weight=gw, g_ref=g_ref, g_cur=g_cur)
        n = float(np.linalg.norm(w[:3] - p))
        check_terms(L, t, w, max(ww, gw) * max(1.0, d, n) ** 2)
        check_terms(L, L.SensorTerms(wheel_weight=ww, p=p, d=d), w, ww * max(1.0, d, n) ** 2)
        check_terms(L, L.SensorTerms(gravity_weight=gw, g_ref=g_ref, g_cur=g_cur), w, gw * 4.0)


def test_odometer_guard_on_both_sides(L):
    p = np.array([1.0, -2.0, 0.5])
    for side in (1.0 - 1e-9, 1.0 + 1e-9, 0.0, 0.5, 2.0):
        u = np.array([0.6, -0.8, 0.0])
        w = np.concatenate([p + u * math.sqrt(1e-6) * side, [0.1, 0.2, 0.3]])
        t = L.SensorTerms(wheel_weight=2.0, p=p, d=0.7)
        got = check_terms(L, t, w, 2.0)
        live = (w[0] - p[0]) ** 2 + (w[1] - p[1]) ** 2 + (w[2] - p[2]) ** 2 >= 1e-6
        assert (np.abs(got[1:28]).max() > 0) == live  # inside the guard: the constant 0, no gradient and no Hessian
        if not live:
            assert got[0] == 0.5 * (2.0 * (0.7 * 0.7))
