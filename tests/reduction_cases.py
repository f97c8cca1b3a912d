"""Residual sets, exact references and a derived error bound for the 29 normal-equation sums of lsa_accumulate
(k_accumulate) and the one-launch solve (k_lm_solve).

A plain module, not a conftest: tests/test_reduction_reference.py checks the reference, the bound and its power to
catch mutated sums on any machine; tests/test_gpu_reduction.py holds both kernels to them at forced launch shapes.

Per-block values.  O.numerics(6, ...) evaluates one residual block with the oracle's restatement of accumulate_one;
tests/test_gpu_numerics.py holds the device's template bit-identical to it, and both kernels build the rotation from
lsa_cos / lsa_sin (lsa_accumulate on the host, k_lm_solve in finish_point).  So these are the very doubles the kernels
add, and the exactly rounded sum of each of the 28 columns (math.fsum) is the reference: it has no error of its own
beyond one rounding.  The count (slot 28 of the product's 29) is an integer and must be equal.

Bound (standard recursive summation, Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., (4.4)): a sum
formed by any tree of floating-point additions in which no term passes through more than d additions satisfies
|S - sum t_i| <= gamma_d * sum |t_i|, gamma_d = d u / (1 - d u), u = 2^-53 (round to nearest; additions of subnormal
numbers are exact, so underflow adds nothing).  fsum = fl(sum t_i) = (sum t_i) / (1 + delta), |delta| <= u, so
|fsum - sum t_i| <= u |fsum|, and together
    |S_dev - fsum| <= gamma_d * sum_i |t_i| + u * |fsum|.
d is read from the code (lsa_accum.h, lsa_accumulate.hip, lsa_lm.hip):
  k_lm_solve    per_thread (the thread's own blocks, acc starts at 0), 6 (wave_reduce_accum: permlane32 swap, permlane16
                swap, row_ror:8, row_half_mirror, two quad_perms), 7 (the 8 wavefronts in LDS), ceil(nb / 8) (the
                strided fold b = j, j + 8, ... from 0), 7 (the 8 partials);
  k_accumulate  per_thread, 6, 3 (the 4 wavefronts), accum_blocks (the host's fold in block order from 0; the device's
                k_accumulate_final folds the same way).
The first addition of each chain starts from 0 and is exact, so d over-counts by a few: the bound stays valid.
"""
import functools
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
NSUMS = 28      # cost, g[6], H upper triangle row by row [21]; the count is compared on its own
D_WIDE = 300    # no shape the GPU tests force needs more (k_accumulate at 256 blocks: 256 + 3 + 6 + 6 = 271)
THREADS_LM, THREADS_ACC = 512, 256


def gamma(d):
    return d * U / (1.0 - d * U)


def depth_lm(nb, per_thread):
    return per_thread + 6 + 7 + -(-nb // 8) + 7


def depth_accum(blocks, per_thread):
    return per_thread + 6 + 3 + blocks


def rot(w):
    """R = Rz Ry Rx of (rx, ry, rz) = w[3:6], numpy libm (for building sets only)"""
    cx, sx, cy, sy, cz, sz = np.cos(w[3]), np.sin(w[3]), np.cos(w[4]), np.sin(w[4]), np.cos(w[5]), np.sin(w[5])
    return np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz], [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz],
                     [-sy, sx * cy, cx * cy]])


def pose_matrix(w):
    T = np.eye(4)
    T[:3, :3] = rot(w)
    T[:3, 3] = w[:3]
    return T


class RSet:
    """Residual blocks of the three keypoint types: status[t] (n_t,), records[t] (n_t, 16) in lsa_download_match's
    layout, sat[t]; points = evaluation points; prior = start point of a solve"""

    def __init__(self, family, label, status, records, sat, points, prior=None):
        self.family, self.label = family, label
        self.status = [np.ascontiguousarray(s, np.uint8) for s in status]
        self.records = [np.ascontiguousarray(r, np.float64).reshape(-1, 16) for r in records]
        self.sat = [float(s) for s in sat]
        self.points = [np.asarray(p, np.float64) for p in points]
        self.prior = np.asarray(points[0] if prior is None else prior, np.float64)

    @property
    def counts(self):
        return tuple(int(s.size) for s in self.status)

    @property
    def total(self):
        return sum(self.counts)

    @property
    def nvalid(self):
        return int(sum(int(np.count_nonzero(s == 0)) for s in self.status))

    def __repr__(self):
        return f"{self.family}[{self.label}] counts {self.counts}"


def block_terms(O, rs, w):
    """(n_valid, 28): every accepted residual block's cost, g, H upper at w, in the product's order (EDGE, PLANE, BLOB)"""
    parts = []
    for t in range(3):
        ok = rs.status[t] == 0
        rec = rs.records[t][ok]
        inp = np.empty((rec.shape[0], 23))
        inp[:, :16] = rec
        inp[:, 16] = rs.sat[t]
        inp[:, 17:] = np.asarray(w, np.float64)
        parts.append(O.numerics(6, inp) if rec.shape[0] else np.zeros((0, NSUMS)))
    return np.concatenate(parts)


def fsum_cols(T):
    # (+ 0.0: an exact zero is +0 in every order the kernels add in, since every chain starts from +0)
    return np.array([math.fsum(T[:, v].tolist()) + 0.0 for v in range(T.shape[1])])


def abs_cols(T):
    return np.array([math.fsum(np.abs(T[:, v]).tolist()) for v in range(T.shape[1])])


class Reference:
    """exact sums of a set at one point, and the per-entry bound at any depth"""

    def __init__(self, O, rs, w):
        self.T = block_terms(O, rs, w)
        self.sums = fsum_cols(self.T)
        self.abs = abs_cols(self.T)
        self.count = self.T.shape[0]

    def bound(self, d):
        return gamma(d) * self.abs + U * np.abs(self.sums)

    def violations(self, S, d):
        """indices of the 28 entries of S outside the bound (NaN counts as outside)"""
        S = np.asarray(S, np.float64)
        return np.flatnonzero(~(np.abs(S - self.sums) <= self.bound(d)))


def sums_of(cost, g, H):
    """the 28 sums in slot order from (cost, g[6], H 6x6)"""
    H = np.asarray(H, np.float64).reshape(6, 6)
    return np.concatenate([[cost], np.asarray(g, np.float64), [H[a, b] for a in range(6) for b in range(a, 6)]])


def split(total, i):
    """type counts of the i-th shape: count[0] in {1, 511, 513}; every other split has an empty middle type"""
    c0 = min((1, 511, 513)[i % 3], total)
    c1 = 0 if i % 2 else (total - c0) // 3
    return (c0, c1, total - c0 - c1)


# ---------------------------------------------------------------------------------------------------------------------
# EXACT: every per-block value is a multiple of 2^-15 and every entry's sum |t_i| < 2^38 (below), so every partial sum
# of any order is representable: all orders give the exact sum bit for bit.
#   w = 0: lsa_cos(0) = 1 and lsa_sin(0) = 0 exactly, R = I, dR entries in {0, +-1}, t = 0.
#   A = diag(d), d in {1/2, 1, 2}; X multiples of 1/8 with |X_i| <= 64; weight 2^-j, j = 0..3.
#   saturation a = 3 * 2^k per type (k = -1, 0, 1): a^2 = 9 * 4^k and a^2 / 3 = 3 * 4^k are exact.
#   one residual component r = 0 (rho' = 1, rho = 0), +-a/2 (s = a^2/4: rho' = 9/16, rho = a^2/3 * 37/64) or +-2a
#   (s > a^2: rho' = 0, rho = a^2/3); P = X - r / d exactly, so A (X - P) = r exactly.
#   J entries: multiples of 1/16, |J| <= 128; H terms (9/16) 2^-j J.J: multiples of 2^-15, <= 3 * 2^14; g terms
#   multiples of 2^-13; cost multiples of 2^-12.  163 840 blocks (the largest set) * 3 * 2^14 < 2^33.
EXACT_K = (-1, 0, 1)


def exact_set(seed, counts, g_zero=False, label=""):
    rng = np.random.default_rng(seed)
    status, records, sats = [], [], []
    for t, n in enumerate(counts):
        a = 3.0 * 2.0 ** EXACT_K[t]
        m = (n + 1) // 2 if g_zero else n
        d = rng.choice([0.5, 1.0, 2.0], size=(m, 3))
        X = rng.integers(-512, 513, size=(m, 3)) / 8.0
        state = rng.integers(0, 3, size=m)
        axis = rng.integers(0, 3, size=m)
        sign = rng.choice([-1.0, 1.0], size=m)
        weight = 2.0 ** -rng.integers(0, 4, size=m).astype(np.float64)
        if g_zero:
            # blocks in pairs with the same J and opposite residuals: the gradient is exactly 0; an unpaired last block
            # has r = 0
            idx = np.repeat(np.arange(m), 2)[:n]
            d, X, state, axis, weight = d[idx], X[idx], state[idx], axis[idx], weight[idx]
            sign = sign[idx] * np.tile([1.0, -1.0], m)[:n]
            if n % 2:
                state[-1] = 0
        rmag = np.where(state == 1, a / 2, np.where(state == 2, 2 * a, 0.0)) * sign
        r = np.zeros((n, 3))
        r[np.arange(n), axis] = rmag
        P = X - r / d
        rec = np.zeros((n, 16))
        rec[:, 0], rec[:, 4], rec[:, 8] = d[:, 0], d[:, 1], d[:, 2]
        rec[:, 9:12], rec[:, 12:15], rec[:, 15] = P, X, weight
        status.append(np.zeros(n, np.uint8))
        records.append(rec)
        sats.append(a)
    return RSet("EXACT0" if g_zero else "EXACT", label, status, records, sats, [np.zeros(6)])


def fraction_terms(rec, sat):
    """accumulate_one at w = 0 in exact rational arithmetic (R = I; dR from rotation_and_derivatives with c = 1, s = 0)"""
    one, zero = Fraction(1), Fraction(0)
    cx = cy = cz = one
    sx = sy = sz = zero
    dRx = [zero, cx * sy * cz + sx * sz, -sx * sy * cz + cx * sz, zero, cx * sy * sz - sx * cz, -sx * sy * sz - cx * cz, zero, cx * cy, -sx * cy]
    dRy = [-sy * cz, sx * cy * cz, cx * cy * cz, -sy * sz, sx * cy * sz, cx * cy * sz, -cy, -sx * sy, -cx * sy]
    dRz = [-cy * sz, -sx * sy * sz - cx * cz, -cx * sy * sz + sx * cz, cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz, zero, zero, zero]

    def mv(M, v):
        return [M[3 * i] * v[0] + M[3 * i + 1] * v[1] + M[3 * i + 2] * v[2] for i in range(3)]

    f = [Fraction(float(v)) for v in rec]
    A, P, X, weight = f[0:9], f[9:12], f[12:15], f[15]
    r = mv(A, [X[i] - P[i] for i in range(3)])
    s = sum(v * v for v in r)
    a2 = Fraction(float(sat)) ** 2
    if s <= a2:
        v = 1 - s / a2
        rho0, rho1 = a2 / 3 * (1 - v ** 3), v ** 2
    else:
        rho0, rho1 = a2 / 3, zero
    rho0, rho1 = rho0 * weight, rho1 * weight
    J = [[A[3 * i + j] for j in range(3)] for i in range(3)]
    for dR in (dRx, dRy, dRz):
        c = mv(A, mv(dR, X))
        for i in range(3):
            J[i].append(c[i])
    out = [rho0 / 2]
    out += [rho1 * sum(J[k][a] * r[k] for k in range(3)) for a in range(6)]
    out += [rho1 * sum(J[k][a] * J[k][b] for k in range(3)) for a in range(6) for b in range(a, 6)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# RANDOM: edge (I - n n^T), plane (n n^T) and blob (inv(B B^T + I)) forms of A from random normals, |X| to ~100 m, P
# about a true pose plus noise of up to 1.6 a (and a sixth of the blocks 2..5 a: beyond a^2), weights 1e-3 .. 1,
# saturations 0.5 .. 10 per type.  Evaluation points: the true pose (translations 0 .. 1e4 m, pitch at +-pi/2 within
# 1e-9 / 1e-12) and a point near it; the solve starts near it.
RANDOM_POSES = (
    ("origin", np.zeros(6)),
    ("t10", np.array([7.0, -4.0, 1.5, 0.4, -0.3, 2.5])),
    ("t1e4", np.array([8.0e3, -6.0e3, 1.2e2, -0.2, 0.1, -2.9])),
    ("pitch+pi/2", np.array([2.0, 1.0, -0.5, 0.7, np.pi / 2 - 1e-9, -1.1])),
    ("pitch-pi/2", np.array([-3.0, 0.5, 0.2, -2.2, -np.pi / 2 + 1e-12, 0.6])),
)
NEAR = np.array([1e-2, -1e-2, 5e-3, 1e-3, -1e-3, 2e-3])


def _random_blocks(rng, n, w, sat, beyond=True):
    nn = rng.normal(size=(n, 3))
    nn /= np.linalg.norm(nn, axis=1)[:, None]
    kind = rng.integers(0, 3, size=n)
    A = np.where((kind == 0)[:, None, None], np.eye(3) - nn[:, :, None] * nn[:, None, :], nn[:, :, None] * nn[:, None, :])
    nb = int(np.count_nonzero(kind == 2))
    if nb:
        B = rng.normal(size=(nb, 3, 3))
        A[kind == 2] = np.linalg.inv(B @ np.transpose(B, (0, 2, 1)) + np.eye(3))
    X = rng.normal(size=(n, 3)) * rng.uniform(1.0, 100.0, size=(n, 1)) / np.sqrt(3.0)
    y = X @ rot(w).T + w[:3]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    mag = rng.uniform(0.0, 1.6, size=n) * sat
    if beyond:
        far = rng.random(n) < 1.0 / 6.0
        mag[far] = rng.uniform(2.0, 5.0, size=int(np.count_nonzero(far))) * sat
    P = y + u * mag[:, None]
    rec = np.zeros((n, 16))
    rec[:, :9] = A.reshape(n, 9)
    rec[:, 9:12], rec[:, 12:15] = P, X
    rec[:, 15] = 10.0 ** rng.uniform(-3.0, 0.0, size=n)
    return rec


def random_set(seed, counts, pose_index, label=""):
    rng = np.random.default_rng(seed)
    name, w = RANDOM_POSES[pose_index % len(RANDOM_POSES)]
    sats = rng.uniform(0.5, 10.0, size=3)
    records = [_random_blocks(rng, n, w, sats[t]) for t, n in enumerate(counts)]
    status = [np.zeros(n, np.uint8) for n in counts]
    prior = w + np.array([0.05, -0.04, 0.03, 0.01, -0.01, 0.02])
    return RSet("RANDOM", f"{label}{name}", status, records, sats, [w, w + NEAR], prior=prior)


# CANCEL: blocks in mirrored pairs about the evaluation point w (P' = 2 (R X + t) - P with R of libm, same A, X, weight):
# the residuals are opposite up to rounding, so g nearly cancels while H and the cost add up.
CANCEL_POSES = (
    ("t10", np.array([3.0, -2.0, 1.0, 0.3, -0.2, 1.5])),
    ("t1e4", np.array([5.0e3, 2.0e3, -40.0, 0.1, 0.2, -0.7])),
)


def cancel_set(seed, counts, pose_index, label=""):
    rng = np.random.default_rng(seed)
    name, w = CANCEL_POSES[pose_index % len(CANCEL_POSES)]
    sats = rng.uniform(0.5, 10.0, size=3)
    R = rot(w)
    records = []
    for t, n in enumerate(counts):
        m = (n + 1) // 2
        base = _random_blocks(rng, m, w, sats[t])
        mir = base.copy()
        mir[:, 9:12] = 2.0 * (base[:, 12:15] @ R.T + w[:3]) - base[:, 9:12]
        rec = np.empty((2 * m, 16))
        rec[0::2], rec[1::2] = base, mir
        records.append(rec[:n])
    status = [np.zeros(n, np.uint8) for n in counts]
    return RSet("CANCEL", f"{label}{name}", status, records, sats, [w], prior=w)


# ---------------------------------------------------------------------------------------------------------------------
# REJECTED: statuses 1..7 over given rows, payloads NaN / +-Inf / 1e308 (what a kernel must never read into a sum), and
# the same set with zero payloads.  Rows are named by their index in the order the kernels walk them (EDGE, PLANE, BLOB).
POISON = np.array([np.nan, np.inf, -np.inf, 1e308])


def reject_rows(total, counts, threads, pattern):
    g = np.arange(total)
    if pattern == "single":
        return g % 97 == 5
    if pattern == "wavefront":  # the second wavefront of the first workgroup and the last whole wavefront of the set
        last = (total // 64 - 1) * 64
        return ((g >= 64) & (g < 128)) | ((g >= last) & (g < last + 64))
    if pattern == "first-row":  # every thread's first residual block (k_lm_solve's register prefetch)
        return g < threads
    if pattern == "type":  # every row of one type
        t = 1 if counts[1] else 0
        lo = sum(counts[:t])
        return (g >= lo) & (g < lo + counts[t])
    raise ValueError(pattern)


REJECT_PATTERNS = ("single", "wavefront", "first-row", "type")


def rejected(rs, mask, zero_payload=False):
    out_s, out_r, lo = [], [], 0
    for t in range(3):
        n = rs.counts[t]
        m = mask[lo:lo + n]
        lo += n
        s, r = rs.status[t].copy(), rs.records[t].copy()
        idx = np.flatnonzero(m)
        s[idx] = 1 + (idx % 7)
        if zero_payload:
            r[idx] = 0.0
        else:
            r[idx] = POISON[(idx[:, None] + np.arange(16)[None, :]) % 4]
        out_s.append(s)
        out_r.append(r)
    return RSet(rs.family + "+REJECTED" + ("0" if zero_payload else ""), rs.label, out_s, out_r, rs.sat, rs.points, rs.prior)


# ---------------------------------------------------------------------------------------------------------------------
# mutants of a sum, applied to the reference's inputs or outputs: the bound at D_WIDE must flag each one in every case
# of RANDOM and CANCEL (tests/test_reduction_reference.py)
STALE = np.array([1e-3, 1e-3, 1e-3, 1e-4, 1e-4, 1e-4])
SWAPS = ((7, 8), (0, 1))  # H(0,0) <-> H(0,1), cost <-> g[0]


def mutant_sums(O, rs, w, ref):
    """[(name, the 28 sums the mutant gives, its count)]; a mutant's sum is the reference plus its change, rounded once
    (an error of u |S|, far below what the bound has to tell apart)"""
    T = ref.T
    out = []

    def changed(delta):
        return np.array([math.fsum([ref.sums[v], float(delta[v])]) for v in range(NSUMS)])

    for v in range(NSUMS):  # the largest term of entry v dropped
        i = int(np.argmax(np.abs(T[:, v])))
        delta = np.zeros(NSUMS)
        delta[v] = -T[i, v]
        out.append((f"drop largest term of entry {v}", changed(delta), ref.count))
    i = int(np.random.default_rng(rs.total).integers(T.shape[0]))  # one block counted twice
    out.append((f"block {i} twice", changed(T[i]), ref.count + 1))
    for a, b in SWAPS:
        S = ref.sums.copy()
        S[a], S[b] = S[b], S[a]
        out.append((f"slots {a} and {b} swapped", S, ref.count))
    # the block with the largest gradient terms evaluated at another point (what a stale exchange would bring)
    i = int(np.argmax(np.abs(T[:, 1:7]).max(axis=1)))
    one = RSet("", "", [np.zeros(1, np.uint8), np.zeros(0, np.uint8), np.zeros(0, np.uint8)], [_row(rs, i), np.zeros((0, 16)), np.zeros((0, 16))],
               [_sat(rs, i), 1.0, 1.0], [w])
    Ti = block_terms(O, one, w + STALE)[0]
    out.append((f"block {i} at another point", changed(Ti - T[i]), ref.count))
    return out


def _row(rs, i):
    t, j = _locate(rs, i)
    return rs.records[t][j:j + 1]


def _sat(rs, i):
    return rs.sat[_locate(rs, i)[0]]


def _locate(rs, i):
    for t in range(3):
        ok = np.flatnonzero(rs.status[t] == 0)
        if i < ok.size:
            return t, int(ok[i])
        i -= ok.size
    raise IndexError(i)


# ---------------------------------------------------------------------------------------------------------------------
# the cases the CPU file checks: the families at sizes and splits of the GPU shapes, built once
CPU_SIZES = (513, 4609, 32767, 163840)


@functools.lru_cache(maxsize=None)
def cpu_cases():
    cases = []
    for i, n in enumerate(CPU_SIZES):
        c = split(n, i)
        for p in range(len(RANDOM_POSES)):
            if n == 163840 and p % 2:
                continue  # the largest size at three of the five poses (the CPU file stays well under a minute)
            cases.append(random_set(1000 + 10 * i + p, c, p, label=f"n{n}-"))
        for p in range(len(CANCEL_POSES)):
            cases.append(cancel_set(2000 + 10 * i + p, c, p, label=f"n{n}-"))
    return cases
