"""Case families and 50-digit mpmath references for the fixed-size solvers behind every match / status / weight decision
and every LM step (lsa_selftest_numerics / oracle.numerics; record layouts in include/lidarslam_amd.h).

A plain module, not a conftest: tests/test_numerics_reference.py checks the oracle's restatements and the product's
host twins against these references on any machine, tests/test_gpu_numerics.py checks the device against the oracle
(bit for bit) and against the same references.  Every family is generated from fixed seeds and built once per process.

Each check returns a list of failure strings "FAMILY case i [label]: what" -- empty when everything holds.  The bounds
and their constants are documented at the check functions and in DESIGN.md 4.4.
"""
import functools
import math

import mpmath  # torch needs sympy, sympy needs mpmath: a missing mpmath is an error, never a skip
import numpy as np

from mpmath import mp, mpf

mp.dps = 50

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}  # unit roundoff
EPS = {np.float32: 2.0 ** -23, np.float64: 2.0 ** -52}  # numeric_limits<T>::epsilon(), the thresholds of eigen33

FN = {"PCA_F": 0, "PCA_D": 1, "EIG33_F": 2, "EIG33_D": 3, "SPD3": 4, "SPD6": 5, "ACCUM": 6, "POSE": 7,
      "SPD3_HOST": 8, "SPD6_HOST": 9, "JACOBI3_HOST": 10, "JACOBI6_HOST": 11}


class Family:
    def __init__(self, name, records, labels, refs):
        self.name = name
        self.records = np.ascontiguousarray(records, np.float64)
        self.labels = labels
        self.refs = refs


def _fmt(fam, i, what):
    return f"{fam} case {i} [{what}]"


# ---------------------------------------------------------------------------------------------------------------------
# small mpmath helpers

def _mpmat(a):
    a = np.asarray(a, np.float64)
    return mp.matrix([[mpf(float(v)) for v in row] for row in a])


def _eigsy(a):
    """ascending eigenvalues (floats) and eigenvectors (columns, float64) of a symmetric matrix, exact input"""
    E, Q = mp.eigsy(_mpmat(a))
    n = a.shape[0]
    lam = [E[i] for i in range(n)]
    order = sorted(range(n), key=lambda i: lam[i])
    vals = np.array([float(lam[i]) for i in order])
    vecs = np.array([[float(Q[r, i]) for i in order] for r in range(n)])
    return vals, vecs


def _gaps(vals):
    n = len(vals)
    return np.array([min([abs(vals[i] - vals[j]) for j in range(n) if j != i]) for i in range(n)])


def _sin_angle(a, b):
    """sin of the angle between two directions, sign-insensitive"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    na, nb = np.linalg.norm(a), np.linalg.norm(b)
    if not (np.isfinite(na) and na > 0):
        return 1.0
    return float(min(1.0, np.linalg.norm(np.cross(a / na, b / nb))))


def _rot(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


# ---------------------------------------------------------------------------------------------------------------------
# PCA: CovAccum<T> + eigen33<T> over k <= 16 float points (PCA_F: line_from_cov of the extractor, PCA_D: the match fits)

def _pca_clouds():
    rng = np.random.default_rng(20261016)
    out = []

    def add(label, pts):
        pts = np.asarray(pts, np.float64).astype(np.float32)
        assert 1 <= len(pts) <= 16
        out.append((label, pts))

    # rank 0
    for k in (2, 5, 16):
        add("rank0-identical", np.tile([[1.5, -2.25, 3.0]], (k, 1)))
        add("rank0-origin", np.zeros((k, 3)))
    add("rank0-identical-far", np.tile([[4096.5, -1023.25, 17.0]], (7, 1)))
    # rank 1: collinear, on an axis and along diagonals
    for k in (2, 3, 8, 16):
        t = rng.uniform(-3, 3, k)
        add("rank1-x-axis", np.stack([t, 0 * t, 0 * t], 1))
        add("rank1-z-axis", np.stack([0 * t, 0 * t, t], 1) + [0, 0, 5])
        add("rank1-diagonal", np.stack([t, t, t], 1))
        add("rank1-diagonal-xy", np.stack([t, -t, 0 * t], 1) + [2, 1, 0])
    # rank 2: coplanar, z = 0 and x = y
    for k in (3, 6, 16):
        a, b = rng.uniform(-2, 2, k), rng.uniform(-2, 2, k)
        add("rank2-plane-z0", np.stack([a, b, 0 * a], 1))
        add("rank2-plane-x=y", np.stack([a, a, b], 1))
        add("rank2-plane-z0-offset", np.stack([a + 30, b - 12, 0 * a + 4], 1))
    # triple eigenvalue (isotropic): the six points +-e_i (cov = I / 3), scaled
    for s in (1.0, 0.5, 8.0, 1e-3):
        e = np.concatenate([np.eye(3), -np.eye(3)]) * s
        add("triple-isotropic", e)
        add("triple-isotropic-offset", e + [3, -2, 1])
    # double eigenvalues: disc (two large equal) and rod (two small equal)
    for s in (1.0, 2.0, 0.25):
        disc = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]]) * s
        add("double-disc", disc)
        add("double-disc-thick", np.concatenate([disc, [[0, 0, 0.25 * s], [0, 0, -0.25 * s]]]))
        rod = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 3], [0, 0, -3]]) * s
        add("double-rod", rod)
    # double eigenvalue symmetric under y <-> z: the isolated eigenvector is (0, 1, -1) / sqrt 2 or (0, 1, 1) / sqrt 2, and
    # the first two cross products of null_vector tie exactly (its >= tie-break decides)
    for p, q, r in ((4, 3, 1), (2, 3, 1), (5, 4, 1), (3, 2, 1)):
        add("double-yz-symmetric", [[p, 0, 0], [-p, 0, 0], [0, q, r], [0, -q, -r], [0, r, q], [0, -r, -q]])
    # eigenvalue gaps straddling eps: +-a e1, +-b e2, +-c e3 with b a few float ulps from a (float path)
    for j in range(0, 6):
        b = np.float32(1.0) + np.float32(j * 2.0 ** -23)
        add(f"gap-l1-l0-{j}ulp", [[1, 0, 0], [-1, 0, 0], [0, b, 0], [0, -b, 0], [0, 0, 2], [0, 0, -2]])
        add(f"gap-l2-l1-{j}ulp", [[0.5, 0, 0], [-0.5, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, b], [0, 0, -b]])
        add(f"gap-l2-l0-{j}ulp", [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, b], [0, 0, -b]])
    # |c0| (the determinant of the scaled matrix) on both sides of eps: a square of side 1, thickness t
    for t in (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 1e-5, 1e-6, 1e-7, 1e-8):
        add(f"c0-thin-{t:g}", [[1, 0, t], [-1, 0, -t], [0, 1, t], [0, -1, -t], [1, 1, -t], [-1, -1, t]])
    # scale <= tiny: spread about 1e-20 (the float products underflow)
    for s in (1e-20, 1e-22, 1e-19):
        add("tiny-spread", rng.normal(size=(8, 3)) * s)
        add("tiny-spread-offset", rng.normal(size=(8, 3)) * s + [1, 2, 3])
    # spreads 1e-3 .. 1e2 m at offsets 0 .. 1e4 m: the one-pass covariance cancels
    for spread in (1e-3, 1e-2, 1e-1, 1.0, 10.0, 100.0):
        for off in (0.0, 10.0, 100.0, 1e3, 1e4):
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            k = int(rng.integers(3, 17))
            shape = np.diag([1.0, 0.3, 0.05]) @ _rot(rng).T
            add(f"offset-{off:g}-spread-{spread:g}", rng.normal(size=(k, 3)) @ shape * spread + off * d)
    # random well-conditioned clouds (control)
    for _ in range(40):
        k = int(rng.integers(4, 17))
        add("random", rng.normal(size=(k, 3)) @ np.diag(rng.uniform(0.5, 2.0, 3)) @ _rot(rng).T + rng.uniform(-5, 5, 3))
    return out


@functools.lru_cache(maxsize=None)
def pca_family():
    recs, labels, refs = [], [], []
    for label, pts in _pca_clouds():
        k = len(pts)
        rec = np.zeros(49)
        rec[0] = k
        rec[1:1 + 3 * k] = pts.astype(np.float64).ravel()
        P = [[mpf(float(v)) for v in p] for p in pts]
        mu = [sum(p[j] for p in P) / k for j in range(3)]
        C = mp.matrix(3, 3)
        for p in P:
            for a in range(3):
                for b in range(3):
                    C[a, b] += (p[a] - mu[a]) * (p[b] - mu[b]) / k
        Cf = np.array([[float(C[a, b]) for b in range(3)] for a in range(3)])
        E, Q = mp.eigsy(C)
        order = sorted(range(3), key=lambda i: E[i])
        vals = np.array([float(E[i]) for i in order])
        vecs = np.array([[float(Q[r, i]) for i in order] for r in range(3)])
        mu_f = np.array([float(m) for m in mu])
        recs.append(rec)
        labels.append(label)
        refs.append(dict(mean=mu_f, vals=vals, vecs=vecs, cov=Cf, norm_c=float(np.max(np.abs(vals))), mu2=float(mu_f @ mu_f),
                         maxabs=float(np.max(np.abs(pts.astype(np.float64)))), k=k, pts=pts))
    return Family("PCA", np.array(recs), labels, refs)


def _computed_scale(pts, dtype):
    """max |cov| as CovAccum<T>::finish forms it (float products, T sums, numpy's IEEE operations in the same order)"""
    T = dtype
    a = [T(0)] * 9
    for x, y, z in pts:
        pr = (x * x, x * y, x * z, y * y, y * z, z * z)  # float32 * float32 = float32
        for j in range(6):
            a[j] = T(a[j] + T(pr[j]))
        a[6], a[7], a[8] = T(a[6] + T(x)), T(a[7] + T(y)), T(a[8] + T(z))
    c = T(len(pts))
    a = [T(v / c) for v in a]
    cov = (a[0] - a[6] * a[6], a[1] - a[6] * a[7], a[2] - a[6] * a[8], a[3] - a[7] * a[7], a[4] - a[7] * a[8], a[5] - a[8] * a[8])
    return float(max(abs(T(v)) for v in cov))


def _eig_bounds(u, S, gaps):
    """per-eigenvalue error bound of eigen33 on a matrix of size S with exact eigenvalue gaps (see C_ROOT)"""
    with np.errstate(divide="ignore"):
        cond = np.minimum(np.where(gaps > 0, S / np.where(gaps > 0, gaps, 1.0), np.inf), 1.0 / math.sqrt(u))
    return C_LAM * u * S + C_ROOT * u * S * cond


def _eig_branch(l, dtype):
    """which branch of eigen33 the returned eigenvalues select (l = scaled eigenvalues, ascending)"""
    eps = EPS[dtype]
    if l[2] - l[0] <= eps:
        return "triple"
    if l[1] - l[0] <= eps:
        return "double-low"
    if l[2] - l[1] <= eps:
        return "double-high"
    return "general"


def _frame_checks(tag, E, dtype, c_ortho):
    """E = columns e0 e1 e2: orthonormal to c_ortho * u, det +1"""
    u = U[dtype]
    f = []
    if not np.all(np.isfinite(E)):
        return [f"{tag}: non-finite eigenvector {E.T.tolist()}"]
    G = E.T @ E - np.eye(3)
    if np.max(np.abs(G)) > c_ortho * u:
        f.append(f"{tag}: frame not orthonormal, |E^T E - I| = {np.max(np.abs(G)):.3g} > {c_ortho} u")
    d = np.linalg.det(E)
    if abs(d - 1.0) > c_ortho * u:
        f.append(f"{tag}: det = {d!r}, not +1")
    return f


# PCA constants.
#  C_LAM: the covariance is a sum of k <= 16 products (one rounding each: float products on BOTH paths, PCL 1.10 forms
#  them from the float members) divided by k, minus mu mu^T: <= (k + 3) u (|C*| + |mu|^2) per entry, then eigen33 on the
#  scaled matrix adds a few u |C*| away from repeated roots.  3 * (16 + 3) + 8 ~ 64.
#  C_MEAN: a sum of k <= 16 values and a division: (k + 1) u max|x| -> 17, rounded up to 20.
#  C_ORTHO: the frame comes from cross products and normalisations of unit vectors: a few ulps each -> 16.
#  C_ROOT: FINDING -- pcl::computeRoots takes the eigenvalues as roots of the characteristic cubic, whose
#  coefficients carry O(u S^3) rounding (S = |C*| + |mu|^2): a root moves by that over p'(lambda) ~ gap S, i.e.
#  u S^2 / gap, and next to a repeated eigenvalue by O(sqrt(u) S) (q = half_b^2 + a^3 cancels, sqrt(-q) = O(sqrt u)).
#  So eigenvalue i is held to C_LAM u S + C_ROOT u S min(S / gap_i, u^-1/2) and eigenvector i to that over gap_i.  A
#  symmetric eigensolver (Jacobi, QR) would meet C u S; this is the reference's algorithm and is kept as is.
#  FINDING -- the float products of coordinates below ~1e-19 m are subnormal: each carries an absolute
#  error of up to half the float quantum 2^-149, on the double path too; F_QUANTUM adds C_LAM such quanta.
#  FINDING -- pcl::eigen33 does not scale a matrix whose largest entry is <= numeric_limits<T>::min()
#  (scale = 1): its characteristic coefficients then underflow and the eigen-decomposition is meaningless.  For those
#  (float spreads below ~1e-19 m) only finiteness, the frame and |lambda - lambda*| <= 4 min() are held.
C_LAM, C_MEAN, C_ORTHO, C_ROOT = 64, 20, 16, 16
PRODUCT_U = np.float32  # both paths form the coordinate products in float
F_QUANTUM = 2.0 ** -149
TINY = {np.float32: float(np.finfo(np.float32).tiny), np.float64: float(np.finfo(np.float64).tiny)}


def check_pca(fam, out, dtype):
    """out: (n, 15) of fn PCA_F (dtype float32) or PCA_D (float64)"""
    u, uprod = U[dtype], U[PRODUCT_U]
    fails = []
    for i, (label, ref, o) in enumerate(zip(fam.labels, fam.refs, out)):
        mean, lam, E = o[0:3], o[3:6], o[6:15].reshape(3, 3).T
        sc = ref["norm_c"] + ref["mu2"]
        scale = _computed_scale(ref["pts"], dtype)
        branch = _eig_branch(lam / (scale if scale > TINY[dtype] else 1.0), dtype)
        tag = _fmt(f"PCA_{'F' if dtype == np.float32 else 'D'}", i, f"{label} / {branch}")
        if not np.all(np.isfinite(o)):
            fails.append(f"{tag}: non-finite output {o.tolist()}")
            continue
        if np.max(np.abs(mean - ref["mean"])) > C_MEAN * u * ref["maxabs"]:
            fails.append(f"{tag}: mean {mean.tolist()} vs {ref['mean'].tolist()}")
        if scale <= TINY[dtype]:  # eigen33 left the matrix unscaled
            err = np.max(np.abs(lam - ref["vals"]))
            if err > 4 * TINY[dtype]:
                fails.append(f"{tag}: unscaled eigenvalues {lam.tolist()} vs {ref['vals'].tolist()}")
            fails += _frame_checks(tag, E, dtype, C_ORTHO)
            continue
        gaps = _gaps(ref["vals"])
        lb = _eig_bounds(uprod, sc, gaps) + C_LAM * F_QUANTUM
        for j in range(3):
            err = abs(lam[j] - ref["vals"][j])
            if err > lb[j]:
                fails.append(f"{tag}: eigenvalue {j} = {lam[j]!r}, reference {ref['vals'][j]!r}: error {err:.3g} > {lb[j]:.3g}")
        fails += _frame_checks(tag, E, dtype, C_ORTHO)
        if branch == "triple":
            if not np.array_equal(E, np.eye(3)):
                fails.append(f"{tag}: triple-eigenvalue branch must return the identity, got {E.T.tolist()}")
            continue
        for j in range(3):
            if gaps[j] == 0.0 or lb[j] / gaps[j] >= 1.0:
                continue  # inside a repeated eigenspace any direction is right
            s = _sin_angle(E[:, j], ref["vecs"][:, j])
            if s > lb[j] / gaps[j]:
                fails.append(f"{tag}: eigenvector {j} off by sin = {s:.3g} > {lb[j] / gaps[j]:.3g} (gap {gaps[j]:.3g})")
    return fails


# ---------------------------------------------------------------------------------------------------------------------
# EIG33: eigen33<T> on a given Sym3 -- sits exactly on the branch boundaries and tie-breaks

def _sym6(M):
    return [M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2]]


def _eig33_mats():
    rng = np.random.default_rng(33)
    out = []
    for dtype in (np.float32, np.float64):
        e = EPS[dtype]
        for j in (0, 0.5, 1, 2, 4):
            out.append((dtype, f"gap-l1-l0-{j}eps", np.diag([1.0, 1.0 + j * e, 0.25])))  # scaled: 0.25, 1, 1 + j eps
            out.append((dtype, f"gap-l2-l1-{j}eps", np.diag([0.25, 1.0 - j * e, 1.0])))
            out.append((dtype, f"gap-l2-l0-{j}eps", np.diag([1.0, 1.0 - j * e / 2, 1.0 - j * e])))
        out.append((dtype, "zero", np.zeros((3, 3))))
        # null_vector's >= tie-break: y <-> z symmetric matrices, the first two cross products tie exactly
        for a, c, d in ((4.0, 3.0, 1.0), (2.0, 3.0, 1.0), (5.0, 3.0, 2.0), (1.0, 3.0, 2.0), (3.0, 2.5, 0.5)):
            out.append((dtype, "tie-yz-symmetric", np.array([[a, 0, 0], [0, c, d], [0, d, c]])))
            out.append((dtype, "tie-yz-symmetric-coupled", np.array([[a, 0.5, 0.5], [0.5, c, d], [0.5, d, c]])))
        # unit_orthogonal's ortho_prec test: isolated eigenvector s = (x, 0, 1) / |.| with |x| next to prec |z|
        prec = 1e-5 if dtype == np.float32 else 1e-12
        for f in (0.5, 0.999, 1.0, 1.001, 2.0):
            for sy in (0.0, 1.0):
                sv = np.array([f * prec, sy * f * prec, 1.0])
                sv /= np.linalg.norm(sv)
                out.append((dtype, f"ortho-prec-{f:g}", np.eye(3) + 2.0 * np.outer(sv, sv)))
                out.append((dtype, f"ortho-prec-{f:g}-low", 3.0 * np.eye(3) - 2.0 * np.outer(sv, sv)))
        # rank 1 and 2 along axes and diagonals
        for v in ([1, 0, 0], [0, 0, 1], [1, 1, 1], [1, -1, 0]):
            v = np.array(v, float)
            out.append((dtype, "rank1", np.outer(v, v)))
            out.append((dtype, "rank2", np.eye(3) * (v @ v) - np.outer(v, v)))
        # indefinite: the r0 <= 0 fall-back to the quadratic (FINDING)
        for lam in ((-1.0, 2.0, 3.0), (-0.5, 1.0, 1.0), (-2.0, -1.0, 4.0), (-1e-3, 1.0, 2.0)):
            Q = _rot(rng)
            out.append((dtype, "indefinite", Q @ np.diag(lam) @ Q.T))
        # random well-separated and clustered spectra
        for _ in range(12):
            Q = _rot(rng)
            out.append((dtype, "random", Q @ np.diag(np.sort(rng.uniform(0.01, 4.0, 3))) @ Q.T))
        for g in (1e-2, 1e-4, 1e-6):
            Q = _rot(rng)
            out.append((dtype, f"cluster-{g:g}", Q @ np.diag([1.0, 1.0 + g, 3.0]) @ Q.T))
    return out


@functools.lru_cache(maxsize=None)
def eig33_family(dtype):
    recs, labels, refs = [], [], []
    for dt, label, M in _eig33_mats():
        if dt is not dtype:
            continue
        s6 = np.array(_sym6(M)).astype(dtype).astype(np.float64)
        Mx = np.array([[s6[0], s6[1], s6[2]], [s6[1], s6[3], s6[4]], [s6[2], s6[4], s6[5]]])
        vals, vecs = _eigsy(Mx)
        ref = dict(vals=vals, vecs=vecs, norm=float(np.max(np.abs(vals))), M=Mx)
        if label == "indefinite":
            # pcl::computeRoots then returns 0 and the roots of x^2 - c2 x + c1 (the 2x2 principal minors)
            m = _mpmat(Mx)
            c2 = m[0, 0] + m[1, 1] + m[2, 2]
            c1 = m[0, 0] * m[1, 1] - m[0, 1] ** 2 + m[0, 0] * m[2, 2] - m[0, 2] ** 2 + m[1, 1] * m[2, 2] - m[1, 2] ** 2
            d = max(c2 * c2 - 4 * c1, mpf(0))
            ref["fallback"] = np.array([0.0, float((c2 - mp.sqrt(d)) / 2), float((c2 + mp.sqrt(d)) / 2)])
        recs.append(s6)
        labels.append(label)
        refs.append(ref)
    return Family(f"EIG33_{'F' if dtype == np.float32 else 'D'}", np.array(recs), labels, refs)


def check_eig33(fam, out, dtype):
    """out: (n, 12).  The input is exact: the PCA bounds with S = |M| and the unit roundoff of T (see C_ROOT)."""
    u = U[dtype]
    fails = []
    for i, (label, ref, o) in enumerate(zip(fam.labels, fam.refs, out)):
        lam, E = o[0:3], o[3:12].reshape(3, 3).T
        nrm = ref["norm"]
        scale = float(np.max(np.abs(ref["M"])))
        branch = _eig_branch(lam / (scale if scale > TINY[dtype] else 1.0), dtype)
        tag = _fmt(fam.name, i, f"{label} / {branch}")
        if not np.all(np.isfinite(o)):
            fails.append(f"{tag}: non-finite output {o.tolist()}")
            continue
        fails += _frame_checks(tag, E, dtype, C_ORTHO)
        if "fallback" in ref:
            err = np.max(np.abs(lam - ref["fallback"]))
            if lam[0] != 0.0 or err > C_LAM * u * nrm:
                fails.append(f"{tag}: indefinite input must give 0 and the quadratic's roots {ref['fallback'].tolist()}, got {lam.tolist()}")
            continue
        if branch == "triple" and not np.array_equal(E, np.eye(3)):
            fails.append(f"{tag}: triple-eigenvalue branch must return the identity, got {E.T.tolist()}")
        gaps = _gaps(ref["vals"])
        lb = _eig_bounds(u, nrm, gaps)
        for j in range(3):
            if abs(lam[j] - ref["vals"][j]) > lb[j]:
                fails.append(f"{tag}: eigenvalue {j} = {lam[j]!r}, reference {ref['vals'][j]!r} (bound {lb[j]:.3g})")
        if branch == "triple":
            continue
        for j in range(3):
            if gaps[j] == 0.0 or lb[j] / gaps[j] >= 1.0:
                continue
            s = _sin_angle(E[:, j], ref["vecs"][:, j])
            if s > lb[j] / gaps[j]:
                fails.append(f"{tag}: eigenvector {j} off by sin = {s:.3g} > {lb[j] / gaps[j]:.3g}")
    return fails


# ---------------------------------------------------------------------------------------------------------------------
# SPD: solve_spd<N> (device) / SolveSPD (host LM loop) / CholeskySolve (oracle)

def _spd_cases(N):
    rng = np.random.default_rng(600 + N)
    out = []
    for logk in range(0, 16):
        for _ in range(3):
            Q, _r = np.linalg.qr(rng.normal(size=(N, N)))
            sig = np.logspace(0, -logk, N) * 10.0 ** rng.uniform(-3, 3)
            out.append((f"cond-1e{logk}", Q @ np.diag(sig) @ Q.T, rng.normal(size=N), True))
    # what LM really solves: Jacobi-scaled J^T J plus lambda diag
    for lam in (1e-8, 1e-4, 1.0, 1e4):
        for _ in range(3):
            J = rng.normal(size=(40, N)) * np.logspace(0, -3, N)
            H = J.T @ J
            D = 1.0 / (1.0 + np.sqrt(np.diag(H)))
            Hs = D[:, None] * H * D[None, :]
            out.append((f"lm-lambda-{lam:g}", Hs + lam * np.diag(np.diag(Hs)), rng.normal(size=N), True))
    # must fail: exactly singular, indefinite, a zero or negative pivot appearing late, NaN / Inf
    v = np.arange(1, N + 1, dtype=float)
    out.append(("singular-rank1", np.outer(v, v), np.ones(N), False))
    out.append(("singular-zero-row", np.diag([1.0] * (N - 1) + [0.0]), np.ones(N), False))
    out.append(("indefinite", np.diag([1.0, -1.0] + [1.0] * (N - 2)), np.ones(N), False))
    A = np.eye(N)
    A[N - 1, N - 1] = -1e-300
    out.append(("late-negative-pivot", A, np.ones(N), False))
    Lf = np.tril(np.ones((N, N)))
    Lf[N - 1, N - 1] = 0.0
    out.append(("late-zero-pivot", Lf @ Lf.T, np.ones(N), False))  # integers: the last pivot is exactly 0
    A = Lf @ Lf.T
    A[N - 1, N - 1] -= 1.0
    out.append(("late-negative-pivot-int", A, np.ones(N), False))
    for bad in (np.nan, np.inf, -np.inf):
        A = np.eye(N) * 2.0
        A[N - 1, N - 1] = bad
        out.append((f"A-diag-{bad}", A, np.ones(N), False))
        A = np.eye(N) * 2.0
        A[N - 1, 0] = A[0, N - 1] = bad
        out.append((f"A-offdiag-{bad}", A, np.ones(N), False))
        b = np.ones(N)
        b[N // 2] = bad
        out.append((f"b-{bad}", np.eye(N) * 2.0, b, False))
    # finite A and b whose solution overflows
    out.append(("x-overflow", np.eye(N) * 1e-300, np.full(N, 1e300), False))
    return out


@functools.lru_cache(maxsize=None)
def spd_family(N):
    recs, labels, refs = [], [], []
    for label, A, b, solvable in _spd_cases(N):
        A = np.asarray(A, np.float64)
        if np.all(np.isfinite(A)):
            A = (A + A.T) / 2
        recs.append(np.concatenate([A.ravel(), b]))
        labels.append(label)
        ref = dict(solvable=solvable)
        if solvable:
            x = mp.lu_solve(_mpmat(A), mp.matrix([mpf(float(v)) for v in b]))
            ref["x"] = np.array([float(x[i]) for i in range(N)])
            ev = _eigsy(A)[0]
            ref["kappa"] = float(ev[-1] / ev[0])
        refs.append(ref)
    return Family(f"SPD{N}", np.array(recs), labels, refs)


# C_SPD: Cholesky's backward error is <= (N + 1) u |A| per entry and the forward error <= kappa times it; 2 (N + 1) + 2 -> 16
C_SPD = 16


def check_spd(fam, out, N):
    u = U[np.float64]
    fails = []
    for i, (label, ref, o) in enumerate(zip(fam.labels, fam.refs, out)):
        ok, x = o[0], o[1:1 + N]
        tag = _fmt(fam.name, i, label)
        if ok not in (0.0, 1.0):
            fails.append(f"{tag}: ok flag {ok!r}")
            continue
        if ok and not np.all(np.isfinite(x)):
            fails.append(f"{tag}: ok with a non-finite x {x.tolist()}")
        if not ref["solvable"]:
            if ok:
                fails.append(f"{tag}: singular / indefinite / non-finite input reported ok, x = {x.tolist()}")
            continue
        if not ok:
            if ref["kappa"] * u < 1e-3:  # comfortably positive definite: Cholesky cannot fail
                fails.append(f"{tag}: not ok (kappa {ref['kappa']:.3g})")
            continue
        err = np.linalg.norm(x - ref["x"]) / np.linalg.norm(ref["x"])
        if err > C_SPD * ref["kappa"] * u:
            fails.append(f"{tag}: |x - x*| / |x*| = {err:.3g} > {C_SPD} kappa u (kappa {ref['kappa']:.3g})")
    return fails


# ---------------------------------------------------------------------------------------------------------------------
# JACOBI (host): SymEigen of host/lsa_lm.cpp / JacobiEigen of the oracle -- the registration-error covariance

def _jacobi_cases(N):
    rng = np.random.default_rng(700 + N)
    out = []
    for top in (0, 2, 4, 8, 12, 16):
        for _ in range(3):
            Q, _r = np.linalg.qr(rng.normal(size=(N, N)))
            out.append((f"spread-1e{top}", Q @ np.diag(np.logspace(top, 0, N) * rng.permutation(N) / N + np.logspace(top, 0, N)) @ Q.T))
    for _ in range(3):
        Q, _r = np.linalg.qr(rng.normal(size=(N, N)))
        lam = np.ones(N)
        lam[: N // 2] = 2.0
        out.append(("repeated", Q @ np.diag(lam) @ Q.T))
        lam = rng.uniform(1, 2, N)
        lam[0] = lam[1] = 0.0
        out.append(("zero-eigenvalues", Q @ np.diag(lam) @ Q.T))
    # rank-deficient information matrix: residuals whose A are all the same plane's n n^T (plane-only scene)
    if N == 6:
        n = np.array([0.0, 0.0, 1.0])
        H = np.zeros((6, 6))
        for _ in range(20):
            X = rng.normal(size=3) * 5
            Jr = np.concatenate([n, np.cross(X, n)])  # d(n . (R X + t)) / d(t, rotation)
            H += np.outer(Jr, Jr)
        out.append(("plane-only", H))
    out.append(("diagonal", np.diag(np.arange(1.0, N + 1))))
    for s in (1e-30, 1e-10, 1e10, 1e30):
        Q, _r = np.linalg.qr(rng.normal(size=(N, N)))
        out.append((f"norm-{s:g}", Q @ np.diag(rng.uniform(0.1, 1, N)) @ Q.T * s))
    return out


@functools.lru_cache(maxsize=None)
def jacobi_family(N):
    recs, labels, refs = [], [], []
    for label, A in _jacobi_cases(N):
        A = (A + A.T) / 2
        vals, vecs = _eigsy(A)
        recs.append(A.ravel())
        labels.append(label)
        refs.append(dict(vals=vals, vecs=vecs, norm=float(np.max(np.abs(vals)))))
    return Family(f"JACOBI{N}", np.array(recs), labels, refs)


# C_JAC: each rotation is backward stable to a few u |A| (c and s to a few ulps), one sweep is N (N - 1) / 2 rotations and
# the solver stops within one sweep of the off-diagonal part reaching 1e-18 |A|: |lambda - lambda*| <= C_JAC n u |A|
# with C_JAC = 8 covers ~10 sweeps of accumulated rounding; V is orthogonal to C_JAC n u, its columns within
# C_JAC n u |A| / gap of the exact eigenvectors.
C_JAC = 8


def check_jacobi(fam, out, N):
    u = U[np.float64]
    fails = []
    for i, (label, ref, o) in enumerate(zip(fam.labels, fam.refs, out)):
        lam, V = o[:N], o[N:].reshape(N, N)
        tag = _fmt(fam.name, i, label)
        if not np.all(np.isfinite(o)):
            fails.append(f"{tag}: non-finite output")
            continue
        bnd = C_JAC * N * u * ref["norm"]
        err = np.max(np.abs(lam - ref["vals"]))
        if err > bnd:
            fails.append(f"{tag}: eigenvalues off by {err:.3g} > {bnd:.3g}")
        orth = np.max(np.abs(V.T @ V - np.eye(N)))
        if orth > C_JAC * N * u:
            fails.append(f"{tag}: V not orthogonal ({orth:.3g})")
        gaps = _gaps(ref["vals"])
        for j in range(N):
            if gaps[j] == 0.0 or bnd / gaps[j] >= 1.0:
                continue
            v, w = V[:, j], ref["vecs"][:, j]
            s = float(np.linalg.norm(v - (v @ w) * w))
            if s > bnd / gaps[j]:
                fails.append(f"{tag}: eigenvector {j} off by {s:.3g} > {bnd / gaps[j]:.3g}")
    return fails


# ---------------------------------------------------------------------------------------------------------------------
# ACCUM: rotation_and_derivatives + accumulate_one -- one residual block's cost, gradient and J^T J

def _mp_rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = mp.cos(rx), mp.sin(rx), mp.cos(ry), mp.sin(ry), mp.cos(rz), mp.sin(rz)
    Rz = mp.matrix([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    Ry = mp.matrix([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = mp.matrix([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    dRz = mp.matrix([[-sz, -cz, 0], [cz, -sz, 0], [0, 0, 0]])
    dRy = mp.matrix([[-sy, 0, cy], [0, 0, 0], [-cy, 0, -sy]])
    dRx = mp.matrix([[0, 0, 0], [0, -sx, -cx], [0, cx, -sx]])
    return Rz * Ry * Rx, Rz * Ry * dRx, Rz * dRy * Rx, dRz * Ry * Rx


def _accum_cases():
    rng = np.random.default_rng(6006)
    out = []
    for kind in ("edge", "plane", "blob"):
        for pitch in (0.0, 0.3, np.pi / 2 - 1e-9, np.pi / 2, -np.pi / 2, -np.pi / 2 + 1e-12):
            for tr in (0.0, 10.0, 1e4):
                n = rng.normal(size=3)
                n /= np.linalg.norm(n)
                A = {"edge": np.eye(3) - np.outer(n, n), "plane": np.outer(n, n)}.get(kind)
                if A is None:
                    B = rng.normal(size=(3, 3))
                    A = np.linalg.inv(B @ B.T + np.eye(3))
                w = np.concatenate([rng.normal(size=3) * tr, [rng.uniform(-3, 3), pitch, rng.uniform(-3, 3)]])
                X = rng.normal(size=3) * 20
                P = rng.normal(size=3) * 0.3 + np.array(w[:3]) + X
                out.append((f"{kind}-pitch-{pitch:.6g}-t-{tr:g}", A, P, X, rng.uniform(0.1, 1.0), rng.choice([0.5, 2.0, 10.0]), w))
    # weight 0, and r^2 exactly at / just below / just above the Tukey a^2 (A = I, X = 0: r = t - P exactly)
    for sat in (0.5, 2.0, 3.0):
        for f, lab in ((1.0, "at"), (1.0 - 2.0 ** -52, "below"), (1.0 + 2.0 ** -52, "above"), (0.5, "inside"), (2.0, "outside")):
            out.append((f"tukey-{lab}-a{sat:g}", np.eye(3), np.zeros(3), np.zeros(3), 1.0, sat, np.array([sat * f, 0, 0, 0, 0, 0.0])))
    out.append(("weight-0", np.eye(3), np.ones(3), np.ones(3), 0.0, 1.0, np.array([0.1, 0.2, 0.3, 0.1, 0.2, 0.3])))
    return out


@functools.lru_cache(maxsize=None)
def accum_family():
    recs, labels, refs = [], [], []
    for label, A, P, X, weight, sat, w in _accum_cases():
        rec = np.concatenate([np.ravel(A), P, X, [weight, sat], w])
        Am = _mpmat(np.reshape(rec[:9], (3, 3)))
        Pm, Xm, tm = (mp.matrix([mpf(float(v)) for v in rec[a:a + 3]]) for a in (9, 12, 17))
        R, dRx, dRy, dRz = _mp_rot(mpf(float(rec[20])), mpf(float(rec[21])), mpf(float(rec[22])))
        r = Am * (R * Xm + tm - Pm)
        s = sum(r[i] ** 2 for i in range(3))
        a2 = mpf(float(rec[16])) ** 2
        wt = mpf(float(rec[15]))
        if s <= a2:
            v = 1 - s / a2
            rho0, rho1 = a2 / 3 * (1 - v ** 3), v ** 2
        else:
            rho0, rho1 = a2 / 3, mpf(0)
        J = mp.matrix(3, 6)
        for a in range(3):
            for b in range(3):
                J[a, b] = Am[a, b]
        for c, dR in enumerate((dRx, dRy, dRz)):
            col = Am * (dR * Xm)
            for a in range(3):
                J[a, 3 + c] = col[a]
        g = [float(wt * rho1 * sum(J[k, a] * r[k] for k in range(3))) for a in range(6)]
        H = [float(wt * rho1 * sum(J[k, a] * J[k, b] for k in range(3))) for a in range(6) for b in range(a, 6)]
        nJ = float(mp.sqrt(sum(J[a, b] ** 2 for a in range(3) for b in range(6))))
        nA = float(mp.sqrt(sum(Am[a, b] ** 2 for a in range(3) for b in range(3))))
        recs.append(rec)
        labels.append(label)
        refs.append(dict(cost=float(wt * rho0 / 2), g=np.array(g), H=np.array(H), nJ=nJ, r=float(mp.sqrt(s)), a2=float(a2), w=float(wt),
                         reach=nA * (np.linalg.norm(X) + np.linalg.norm(w[:3]) + np.linalg.norm(P)), inside=bool(s <= a2)))
    return Family("ACCUM", np.array(recs), labels, refs)


# C_ACC: r = A (R X + t - P) is formed with ~8 roundings of quantities of size |A| (|X| + |t| + |P|) =: reach (the
# cancellation of a residual far from the origin is inherent to the formula, not slack): dr <= C_ACC u reach.
# Then g = w rho' J^T r and H = w rho' J^T J carry a few more u relative to w |J| (|r| + dr) and w |J|^2, plus the
# change of rho' = (1 - s / a^2)^2 with s: <= 4 dr / a.  cost = w rho / 2 moves by w (u a^2 + a dr).  C_ACC = 32.
C_ACC = 32


def check_accum(fam, out):
    u = U[np.float64]
    fails = []
    for i, (label, ref, o) in enumerate(zip(fam.labels, fam.refs, out)):
        tag = _fmt("ACCUM", i, label)
        if not np.all(np.isfinite(o)):
            fails.append(f"{tag}: non-finite output")
            continue
        a = math.sqrt(ref["a2"])
        dr = C_ACC * u * (ref["reach"] + ref["r"])
        w, nJ = ref["w"], ref["nJ"]
        drho = 4 * dr / a if ref["inside"] or ref["r"] - dr <= a else 0.0
        checks = (("cost", abs(o[0] - ref["cost"]), C_ACC * w * (u * ref["a2"] + a * dr)),
                  ("g", np.max(np.abs(o[1:7] - ref["g"])), C_ACC * w * nJ * (u * ref["r"] + dr + drho * ref["r"])),
                  ("H", np.max(np.abs(o[7:28] - ref["H"])), C_ACC * w * nJ * nJ * (u + drho)))
        for what, err, bnd in checks:
            if err > bnd:
                fails.append(f"{tag}: {what} off by {err:.3g} > {bnd:.3g}")
    return fails


# ---------------------------------------------------------------------------------------------------------------------
# POSE: the pose algebra between two ICP iterations (lsa_posemath.h / orc_math.hpp)

def _mp_quat_of(R):
    """unit quaternion (w x y z, w >= 0) of an exact rotation matrix (mp)"""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    cands = [(tr, 0), (R[0, 0], 1), (R[1, 1], 2), (R[2, 2], 3)]
    _, k = max(cands, key=lambda c: c[0])
    if k == 0:
        w = mp.sqrt(1 + tr) / 2
        q = [w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)]
    else:
        i = k - 1
        j, l = (i + 1) % 3, (i + 2) % 3
        v = [0, 0, 0]
        v[i] = mp.sqrt(1 + R[i, i] - R[j, j] - R[l, l]) / 2
        v[j] = (R[j, i] + R[i, j]) / (4 * v[i])
        v[l] = (R[l, i] + R[i, l]) / (4 * v[i])
        q = [(R[l, j] - R[j, l]) / (4 * v[i])] + v
    return q if q[0] >= 0 else [-c for c in q]


def _mp_quat_mat(q):
    w, x, y, z = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _mp_slerp(qa, qb, s):
    d = sum(a * b for a, b in zip(qa, qb))
    if d < 0:
        qb, d = [-c for c in qb], -d
    if d >= 1:  # rounded unit quaternions may have d > 1: the limit of the arc is the chord
        return [(1 - s) * a + s * b for a, b in zip(qa, qb)]
    th = mp.acos(d)
    s0, s1 = mp.sin((1 - s) * th) / mp.sin(th), mp.sin(s * th) / mp.sin(th)
    return [s0 * a + s1 * b for a, b in zip(qa, qb)]


def _axis_angle_quat(axis, ang):
    axis = np.asarray(axis, float)
    ax = [mpf(float(v)) for v in axis / np.linalg.norm(axis)]
    n = mp.sqrt(sum(v * v for v in ax))
    return [mp.cos(ang / 2)] + [mp.sin(ang / 2) * v / n for v in ax]


def _pose_cases():
    rng = np.random.default_rng(777)
    out = []
    hp = mp.pi / 2
    # (label, exact quaternion of M0, of M1, w (rpy for FromXYZRPY), qa, qb, s, t, t0, t1)
    def rq():
        return _axis_angle_quat(rng.normal(size=3), mpf(float(rng.uniform(0, math.pi))))
    ulp = 2.0 ** -52
    for k in (-3, -1, 0, 1, 3):
        for sign in (1, -1):
            p = float(sign * hp) + k * ulp * 1.5
            out.append((f"pitch-{'+' if sign > 0 else '-'}pi/2{k:+d}ulp", [0.3, p, -1.2]))
    for p in (0.0, 0.7, -1.2, 1.5707, -1.5707, float(hp) - 1e-7, float(hp) - 1e-5):
        out.append((f"pitch-{p:.7g}", [rng.uniform(-3, 3), p, rng.uniform(-3, 3)]))
    cases = []
    for label, rpy in out:
        cases.append((f"rpy-{label}", dict(rpy=rpy)))
    # rotations by pi about each axis and about diagonals: the branches of ToQuaternionLargest
    for axis in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 1, 1], [0, -1, 1], [1, 0, -1]):
        cases.append((f"pi-about-{axis}", dict(q0=_axis_angle_quat(axis, mp.pi))))
        cases.append((f"near-pi-about-{axis}", dict(q0=_axis_angle_quat(axis, mp.pi - mpf("1e-9")))))
    for ang in ("0", "1e-300", "1e-12", "1e-6", "0.5", "2"):
        cases.append((f"angle-{ang}", dict(q0=_axis_angle_quat(rng.normal(size=3), mpf(ang)))))
    # slerp: d < 0, |d| on both sides of 1 - eps, s in {0, 1} and outside [0, 1]
    for sv in (0.0, 1.0, 0.5, -0.25, 1.75, 0.3):
        qa = rq()
        cases.append((f"slerp-s{sv:g}", dict(qa=qa, qb=rq(), s=sv)))
        cases.append((f"slerp-d<0-s{sv:g}", dict(qa=qa, qb=[-c for c in rq()], s=sv)))
        for dth in ("1e-9", "2e-8", "1.5e-8", "1e-7"):
            qb = _mp_mul(qa, _axis_angle_quat(rng.normal(size=3), mpf(dth)))
            cases.append((f"slerp-near-{dth}-s{sv:g}", dict(qa=qa, qb=qb, s=sv)))
            cases.append((f"slerp-near-{dth}-d<0-s{sv:g}", dict(qa=qa, qb=[-c for c in qb], s=sv)))
    # interpolation within (and outside) a frame's time range
    for tv in (0.0, 0.1, 0.05, -0.02, 0.13):
        cases.append((f"interp-t{tv:g}", dict(q0=rq(), q1=rq(), t=tv, t0=0.0, t1=0.1, tr=True)))
    cases.append(("interp-same-time", dict(q0=rq(), q1=rq(), t=0.05, t0=0.1, t1=0.1, tr=True)))
    return cases


def _mp_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return [aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx]


@functools.lru_cache(maxsize=None)
def pose_family():
    rng = np.random.default_rng(778)
    recs, labels, refs = [], [], []
    for label, c in _pose_cases():
        rpy = c.get("rpy", [0.1, 0.2, 0.3])
        rpy_m = [mpf(float(v)) for v in rpy]
        Rw = _mp_rot(*rpy_m)[0]
        q0 = c.get("q0", _mp_quat_of(Rw))
        q1 = c.get("q1", _axis_angle_quat([0, 0, 1], mpf("0.1")))
        R0, R1 = _mp_quat_mat(q0), _mp_quat_mat(q1)
        t0v = rng.normal(size=3) * (100 if c.get("tr") else 1)
        t1v = t0v + rng.normal(size=3)
        M0 = [float(R0[i, j]) for i in range(3) for j in range(3)] + list(t0v)
        M1 = [float(R1[i, j]) for i in range(3) for j in range(3)] + list(t1v)
        qa = c.get("qa", q0)
        qb = c.get("qb", q1)
        qa_f = [float(v) for v in qa]
        qb_f = [float(v) for v in qb]
        s, tt, tt0, tt1 = c.get("s", 0.4), c.get("t", 0.04), c.get("t0", 0.0), c.get("t1", 0.1)
        rec = np.array(M0 + M1 + [1.0, -2.0, 3.0] + list(rpy) + qa_f + qb_f + [s, tt, tt0, tt1])
        # references, from the rounded inputs where the operation reads them
        M0m = mp.matrix([[mpf(M0[3 * i + j]) for j in range(3)] for i in range(3)])
        ref = dict(R_w=np.array([[float(Rw[i, j]) for j in range(3)] for i in range(3)]))
        r20 = M0m[2, 0]
        ref["gimbal"] = abs(abs(float(-mp.asin(max(min(r20, 1), -1)))) - math.pi / 2) < 1e-6
        ref["rpy_nan"] = abs(r20) > 1
        if not ref["rpy_nan"]:
            ref["rpy"] = np.array([float(mp.atan2(M0m[2, 1], M0m[2, 2])), float(-mp.asin(r20)), float(mp.atan2(M0m[1, 0], M0m[0, 0]))])
        ref["R0"] = np.array([[float(R0[i, j]) for j in range(3)] for i in range(3)])
        ref["q0"] = np.array([float(v) for v in q0])
        ref["angle"] = float(2 * mp.atan2(mp.sqrt(q0[1] ** 2 + q0[2] ** 2 + q0[3] ** 2), abs(q0[0])))
        qam = [mpf(v) for v in qa_f]
        qbm = [mpf(v) for v in qb_f]
        d = abs(sum(a * b for a, b in zip(qam, qbm)))
        th = mp.acos(min(d, 1))
        ref["slerp"] = np.array([float(v) for v in _mp_slerp(qam, qbm, mpf(s))])
        ref["slerp_theta"] = float(th)
        ref["slerp_linear"] = bool(float(d) >= 1.0 - 2.0 ** -52)
        ref["s"] = s
        if tt0 == tt1:
            ref["interp"] = None
        else:
            tau = (mpf(tt) - tt0) / (mpf(tt1) - tt0)
            qi = _mp_slerp(q0, q1, tau)
            Ri = _mp_quat_mat(qi)
            ref["interp"] = np.array([float(Ri[i, j]) for i in range(3) for j in range(3)] +
                                     [float(mpf(a) + tau * (mpf(b) - mpf(a))) for a, b in zip(t0v, t1v)])
            ref["tau"] = float(tau)
            ref["tscale"] = float(np.linalg.norm(t0v) + np.linalg.norm(t1v))
        recs.append(rec)
        labels.append(label)
        refs.append(ref)
    return Family("POSE", np.array(recs), labels, refs)


# C_POSE: a rotation from three half-angle sines / cosines (<= 1 ulp each, lsa_pmath.h) and two quaternion products is
# within ~10 u per entry; the slerp adds the acos / sin of lsa_pmath.h and a division: C_POSE = 32.  In the linear branch
# (|d| >= 1 - eps) slerp is replaced by the chord: its error is O(theta^2) on top.  Angles are held to C_POSE u
# absolutely (the inputs are rounded rotations: atan2 / asin of entries with u errors), except within 1e-6 of
# |pitch| = pi/2 where roll and yaw lose their meaning (gimbal lock) and only the reconstructed matrix is checked --
# FINDING: that reconstruction is within C_POSE u / cos(pitch), not u (IsometryToXYZRPY's atan2 of two
# entries of size cos(pitch)).
C_POSE = 32


def check_pose(fam, out):
    u = U[np.float64]
    fails = []
    for i, (label, ref, o) in enumerate(zip(fam.labels, fam.refs, out)):
        tag = _fmt("POSE", i, label)
        R = o[0:9].reshape(3, 3)
        if np.max(np.abs(R - ref["R_w"])) > C_POSE * u or not np.array_equal(o[9:12], [1.0, -2.0, 3.0]):
            fails.append(f"{tag}: FromXYZRPY off by {np.max(np.abs(R - ref['R_w'])):.3g}")
        rpy = o[15:18]
        if ref["rpy_nan"]:
            # |R20| rounded past 1: asin is NaN, as in the reference (std::asin); only the pitch may be NaN
            if not np.isnan(rpy[1]):
                fails.append(f"{tag}: |R20| > 1 must give a NaN pitch (reference-faithful), got {rpy.tolist()}")
        elif ref["gimbal"]:
            Rb = _mp_rot(*[mpf(float(v)) for v in rpy])[0]
            Rb = np.array([[float(Rb[a, b]) for b in range(3)] for a in range(3)])
            cp = max(math.cos(float(ref["rpy"][1])), u)
            err = np.max(np.abs(Rb - np.asarray(fam.records[i][0:9]).reshape(3, 3)))
            if err > min(2.0, C_POSE * u / cp):
                fails.append(f"{tag}: gimbal-lock reconstruction off by {err:.3g} > {C_POSE} u / cos(pitch)")
        else:
            err = np.max(np.abs(rpy - ref["rpy"]))
            if err > C_POSE * u:
                fails.append(f"{tag}: RPY off by {err:.3g} > {C_POSE} u: {rpy.tolist()} vs {ref['rpy'].tolist()}")
        q = o[18:22]
        err = min(np.max(np.abs(q - ref["q0"])), np.max(np.abs(q + ref["q0"])))
        if err > C_POSE * u:
            fails.append(f"{tag}: ToQuaternion off by {err:.3g}: {q.tolist()} vs {ref['q0'].tolist()}")
        sl = o[22:26]
        bnd = C_POSE * u * (1 + abs(ref["s"])) + (C_POSE * ref["slerp_theta"] ** 2 * (1 + abs(ref["s"])) if ref["slerp_linear"] else 0.0)
        err = np.max(np.abs(sl - ref["slerp"]))
        if not err <= bnd:
            fails.append(f"{tag}: Slerp off by {err:.3g} > {bnd:.3g}: {sl.tolist()} vs {ref['slerp'].tolist()}")
        if not abs(o[26] - ref["angle"]) <= C_POSE * u:
            fails.append(f"{tag}: RotationAngle {o[26]!r} vs {ref['angle']!r}")
        if ref["interp"] is None:
            # Time0 == Time1: the interpolator is invalid and returns H0 as its quaternion gives it back
            if np.max(np.abs(o[27:36] - ref["R0"].ravel())) > C_POSE * u:
                fails.append(f"{tag}: invalid interpolator must return H0")
        else:
            tb = C_POSE * u * (1 + abs(ref["tau"]))
            err_r = np.max(np.abs(o[27:36] - ref["interp"][:9]))
            err_t = np.max(np.abs(o[36:39] - ref["interp"][9:]))
            if err_r > tb or err_t > tb * ref["tscale"]:
                fails.append(f"{tag}: interpolated pose off by {err_r:.3g} (R), {err_t:.3g} (t)")
    return fails
