"""An independent statement of the LM solve's trust-region loop, and the scripts that walk every branch of it.

The loop of LocalOptimizer::Solve reads, per evaluation, 29 sums (cost, g[6], the upper triangle of H = J^T J row by row,
the number of residual blocks), its own state, max_iter and min_matches -- nothing else.  lsa_selftest_lm_step feeds the
device's step (lm_step of lsa_lm.hip) with scripted sums, lsa_selftest_lm_host the host loop (host/lsa_lm_loop.cpp).
`Reference` below is the same loop written from the rules of Ceres's Levenberg-Marquardt trust-region minimizer
(trust_region_minimizer.cc, levenberg_marquardt_strategy.cc; Solver::Options defaults, named below) in plain float64:

  * iteration 0: the evaluation at the start point; fewer residual blocks than min_matches: nothing is optimised.  Jacobi
    scaling once, s_a = 1 / (1 + sqrt(H_aa)); gradient tolerance on max |g_a| (a gradient with a NaN has not converged);
  * every iteration: max_num_iterations, gradient tolerance, min_trust_region_radius, in this order; then the LM diagonal
    D_a = clamp(Hs_aa, min_lm_diagonal, max_lm_diagonal) (kept while steps are rejected), the damped system
    (Hs + D / radius) y = gs by Cholesky, step = -y, model_cost_change = -step . (gs + Hs step / 2);
  * a failed factorization, a non-finite solution or a negative model_cost_change is an invalid step: the radius shrinks,
    max_num_consecutive_invalid_steps of them end the solve, a valid step resets the count;
  * parameter tolerance, then function tolerance, decided before the candidate is taken; relative_decrease =
    cost_change / model_cost_change > min_relative_decrease accepts: radius / max(1/3, 1 - (2 rho - 1)^3), at most
    max_trust_region_radius; otherwise radius / decrease_factor, decrease_factor * 2.

Part of the contract, documented above lm_step, are the ORDERS of the sums, so that the comparison is `==` on bit patterns
(-ffp-contract=off, IEEE sqrt and division): Hs_ab = (H_ab s_a) s_b; the factor row by row, every entry subtracting its
products with k ascending and multiplying by the reciprocal of the pivot; both substitutions with k ascending; s.g and
s.Hs added in index order.  Everything else here is written from the rules, not from the code under test.

The upper clamp of the LM diagonal has no case: Hs_aa = H_aa / (1 + sqrt(H_aa))^2 < 1 for every finite H_aa >= 0, H_aa = inf
gives s_a = 0 and Hs_aa = inf * 0 = NaN, a negative H_aa gives NaN: no sums lead to Hs_aa > 1e32.

Scripts are generated closed-loop on the reference: a `source` is asked for the sums at the reference's candidate
(problem cases: an analytic least-squares problem evaluated with numpy) or composes them from the reference's state
(branch cases: the next cost from its model_cost_change).  In 2D mode the rows and columns z, rx, ry of g and H are NaN and
z, rx, ry of the start point are not 0.
"""
import functools

import numpy as np

F = np.float64

# ceres::Solver::Options defaults
INITIAL_TRUST_REGION_RADIUS = 1e4
MAX_TRUST_REGION_RADIUS = 1e16
MIN_TRUST_REGION_RADIUS = 1e-32
MIN_RELATIVE_DECREASE = 1e-3
MIN_LM_DIAGONAL = 1e-6
MAX_LM_DIAGONAL = 1e32
MAX_NUM_CONSECUTIVE_INVALID_STEPS = 5
FUNCTION_TOLERANCE = 1e-6
GRADIENT_TOLERANCE = 1e-10
PARAMETER_TOLERANCE = 1e-8

# lsa_solve_result_t::termination
NONE, NOT_ENOUGH_MATCHES, GRADIENT0, MAX_ITERATIONS, GRADIENT, MIN_RADIUS, INVALID_STEPS, PARAMETER, FUNCTION = range(9)
CODE_NAMES = ["none", "not enough matches", "gradient tolerance (iteration 0)", "max iterations", "gradient tolerance", "min trust region radius",
              "too many invalid steps", "parameter tolerance", "function tolerance"]

RECORD, RESULT, SUMS = 42, 45, 29
ACTIVE_3D, ACTIVE_2D = (0, 1, 2, 3, 4, 5), (0, 1, 5)


def hidx(a, b):
    """index of H(a, b) in the 29 sums"""
    a, b = min(a, b), max(a, b)
    return 7 + a * 6 - (a * (a - 1)) // 2 + (b - a)


def cholesky_solve(M, b, n):
    """(ok, x) with M x = b; M: its lower triangle is read.  The sum orders of the contract."""
    L = [[F(0)] * n for _ in range(n)]
    rinv = [F(0)] * n
    for i in range(n):
        for j in range(i + 1):
            s = M[i][j]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                if not (s > 0 and np.isfinite(s)):
                    return False, None
                L[i][i] = np.sqrt(s)
                rinv[i] = F(1) / L[i][i]
            else:
                L[i][j] = s * rinv[j]
    y = [F(0)] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s * rinv[i]
    x = [F(0)] * n
    for i in reversed(range(n)):
        s = y[i]
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s * rinv[i]
    return bool(all(np.isfinite(v) for v in x)), x


class Reference:
    """The loop, one evaluation at a time: feed(sums) decides on the candidate the sums were taken at and returns the
    record of 42 doubles (include/lidarslam_amd.h); `candidate` is where the next sums are wanted, `code` how it ended.
    `trace` keeps, per evaluation, what the branch assertions ask about; `systems` every damped system that was solved."""

    def __init__(self, two_d, max_iter, min_matches, x0):
        self.act = ACTIVE_2D if two_d else ACTIVE_3D
        self.n = len(self.act)
        self.max_iter, self.min_matches = int(max_iter), int(min_matches)
        self.x = [F(v) for v in x0]
        self.radius, self.decrease_factor = F(INITIAL_TRUST_REGION_RADIUS), F(2)
        self.x_norm = self.model_cost_change = self.step_norm = self.initial_cost = F(0)
        self.reuse_diagonal, self.invalid, self.iteration = False, 0, 0
        self.evaluations, self.successful, self.unsuccessful, self.skipped, self.matches = 1, 0, 0, False, 0
        self.scale, self.diag = [F(1)] * 6, [F(0)] * 6
        self.adopted = 0
        self.current = np.zeros(SUMS)  # the sums at the current point
        self.code, self.candidate = NONE, None
        self.trace, self.systems, self.records = [], [], []

    # ---- pieces
    def _adopt(self, sums):
        act = self.act
        self.current = np.array(sums, F)
        self.adopted += 1
        self.cost = sums[0]
        self.g = [sums[1 + p] for p in act]
        self.H = [[sums[hidx(p, q)] for q in act] for p in act]

    def _scale_system(self):
        n, s = self.n, self.scale
        self.gs = [self.g[a] * s[a] for a in range(n)]
        self.Hs = [[(self.H[a][b] * s[a]) * s[b] for b in range(n)] for a in range(n)]

    def _gradient_converged(self):
        return bool(all(abs(v) <= GRADIENT_TOLERANCE for v in self.g))

    def _norm(self, v):
        s = F(0)
        for p in self.act:
            s = s + v[p] * v[p]
        return np.sqrt(s)

    def _stop(self, code, t):
        self.code, self.candidate = code, None
        t["decision"] = t.get("decision", "stop")

    # ---- what became of the candidate
    def _decide(self, sums, t):
        cost = sums[0]
        if not self.trace[:-1]:  # the evaluation at the start point
            self.matches = int(sums[28])
            if self.matches < self.min_matches:
                self.skipped = True
                return self._stop(NOT_ENOUGH_MATCHES, t)
            self._adopt(sums)
            self.initial_cost, self.successful = cost, 1
            for a in range(self.n):
                self.scale[a] = F(1) / (F(1) + np.sqrt(self.H[a][a]))
            self._scale_system()
            t["decision"] = "start"
            if self._gradient_converged():
                return self._stop(GRADIENT0, t)
            self.x_norm = self._norm(self.x)
            return
        if self.step_norm <= F(PARAMETER_TOLERANCE) * (self.x_norm + F(PARAMETER_TOLERANCE)):
            return self._stop(PARAMETER, t)
        cost_change = self.cost - cost
        if abs(cost_change) <= F(FUNCTION_TOLERANCE) * self.cost:
            return self._stop(FUNCTION, t)
        rho = cost_change / self.model_cost_change
        t["relative_decrease"] = rho
        if rho > MIN_RELATIVE_DECREASE:
            t["decision"] = "accept"
            self.x = list(self.candidate)
            self.x_norm = self._norm(self.x)
            self._adopt(sums)
            self._scale_system()
            self.successful += 1
            u = F(2) * rho - F(1)
            q = F(1) - u * u * u
            third = F(1) / F(3)
            r = self.radius / (q if third < q else third)
            t["unclamped_radius"] = r
            self.radius = r if r < MAX_TRUST_REGION_RADIUS else F(MAX_TRUST_REGION_RADIUS)
            self.decrease_factor, self.reuse_diagonal = F(2), False
        else:
            t["decision"] = "reject"
            self.unsuccessful += 1
            self.radius = self.radius / self.decrease_factor
            self.decrease_factor = self.decrease_factor * F(2)
            self.reuse_diagonal = True

    # ---- the damped solve and the next candidate
    def _next_candidate(self, t):
        n = self.n
        while True:
            if self.iteration >= self.max_iter:
                return self._stop(MAX_ITERATIONS, t)
            if self._gradient_converged():
                return self._stop(GRADIENT, t)
            if self.radius < MIN_TRUST_REGION_RADIUS:
                return self._stop(MIN_RADIUS, t)
            self.iteration += 1
            if not self.reuse_diagonal:
                for a in range(n):
                    h = self.Hs[a][a]
                    if h < MIN_LM_DIAGONAL:
                        h = F(MIN_LM_DIAGONAL)
                        t["clamped_low"] = t.get("clamped_low", []) + [a]
                    elif h > MAX_LM_DIAGONAL:
                        h = F(MAX_LM_DIAGONAL)
                        t["clamped_high"] = t.get("clamped_high", []) + [a]
                    self.diag[a] = h
            M = [[self.Hs[i][j] + self.diag[i] / self.radius if i == j else self.Hs[i][j] for j in range(n)] for i in range(n)]
            ok, y = cholesky_solve(M, self.gs, n)
            self.reuse_diagonal = True
            self.systems.append((M, list(self.gs), ok, y))
            t["radii_tried"] = t.get("radii_tried", []) + [self.radius]
            if ok:
                step = [-v for v in y]
                sg = sHs = F(0)
                for a in range(n):
                    sg = sg + step[a] * self.gs[a]
                    row = F(0)
                    for b in range(n):
                        row = row + self.Hs[a][b] * step[b]
                    sHs = sHs + step[a] * row
                change = -sg - F(0.5) * sHs
                if change < 0:
                    ok = False
                    t["negative_model_cost_change"] = True
            if not ok:
                self.unsuccessful += 1
                self.invalid += 1
                t["invalid"] += 1
                if self.invalid >= MAX_NUM_CONSECUTIVE_INVALID_STEPS:
                    return self._stop(INVALID_STEPS, t)
                self.radius = self.radius / self.decrease_factor
                self.decrease_factor = self.decrease_factor * F(2)
                continue
            self.invalid = 0
            self.model_cost_change = change
            cand, dn = list(self.x), F(0)
            for a, p in enumerate(self.act):
                cand[p] = self.x[p] + step[a] * self.scale[a]
                e = self.x[p] - cand[p]
                dn = dn + e * e
            self.step_norm = np.sqrt(dn)
            self.evaluations += 1
            self.candidate = cand
            return

    def feed(self, sums):
        assert self.code == NONE, "the solve is over"
        sums = np.array(sums, F)
        t = {"invalid": 0}
        self.trace.append(t)
        with np.errstate(all="ignore"):
            self._decide(sums, t)
            if self.code == NONE:
                self._next_candidate(t)
        t.update(code=self.code, radius=self.radius, consecutive_invalid=self.invalid, diag=list(self.diag[:self.n]), iteration=self.iteration)
        rec = self.record()
        self.records.append(rec)
        return rec

    def record(self):
        o = np.zeros(RECORD)
        if self.candidate is not None:
            o[0:6] = self.candidate
        o[6], o[7] = self.code, self.code != NONE
        o[8:14] = [self.radius, self.decrease_factor, self.x_norm, self.model_cost_change, self.step_norm, self.initial_cost]
        o[14:23] = [self.reuse_diagonal, self.invalid, self.iteration, self.evaluations, self.successful, self.unsuccessful, self.iteration,
                    self.skipped, self.matches]
        o[23:29], o[29:35], o[35:41] = self.x, self.scale, self.diag
        o[41] = self.adopted & 1
        return o

    def result(self):
        o = np.zeros(RESULT)
        o[0:6] = self.x
        o[6], o[7] = self.initial_cost, self.current[0]
        o[8:37] = self.current
        o[37:44] = [self.successful, self.unsuccessful, self.iteration, self.evaluations, self.skipped, self.code, self.matches]
        return o


# ---------------------------------------------------------------------------------------------------------------------
# composing sums

def pack(two_d, cost, g, H, count=1000):
    """29 sums from the active parameters' gradient (n) and matrix (n, n); in 2D mode the inactive entries are NaN"""
    act = ACTIVE_2D if two_d else ACTIVE_3D
    out = np.full(SUMS, np.nan)
    out[0], out[28] = cost, count
    for a, p in enumerate(act):
        out[1 + p] = g[a]
        for b, q in enumerate(act):
            if p <= q:
                out[hidx(p, q)] = H[a][b]
    return out


def start_point(two_d, active):
    """a start point from the active parameters' values; z, rx, ry are not 0 in 2D mode"""
    if not two_d:
        return np.array(active, F)
    return np.array([active[0], active[1], 0.7, -0.3, 0.2, active[2]], F)


def active_of(two_d, point):
    return np.array([point[p] for p in (ACTIVE_2D if two_d else ACTIVE_3D)], F)


class Quadratic:
    """cost = floor + (x - x*)^T H (x - x*) / 2 over the active parameters, H = J^T J of a fixed J"""

    def __init__(self, n, seed, xstar, floor=0.0, column_scales=None):
        rng = np.random.default_rng(seed)
        J = rng.normal(size=(30, n))
        if column_scales is not None:
            J = J * np.asarray(column_scales)[None, :]
        self.H, self.xstar, self.floor = J.T @ J, np.asarray(xstar, F), floor

    def sums(self, two_d, point, count=1000):
        d = active_of(two_d, point) - self.xstar
        g = self.H @ d
        return pack(two_d, self.floor + 0.5 * float(d @ g), g, self.H, count)


class Valley:
    """Rosenbrock's curved valley in the first two active parameters, r = (10 (b - a^2), 1 - a), the others r = v"""

    def sums(self, two_d, point, count=1000):
        v = active_of(two_d, point)
        n = v.size
        r = np.concatenate([[10.0 * (v[1] - v[0] ** 2), 1.0 - v[0]], v[2:]])
        J = np.zeros((n, n))
        J[0, 0], J[0, 1], J[1, 0] = -20.0 * v[0], 10.0, -1.0
        for i in range(2, n):
            J[i, i] = 1.0
        return pack(two_d, 0.5 * float(r @ r), J.T @ r, J.T @ J, count)


class Slope:
    """gradient and matrix that do not depend on the point but on the evaluation's number (a rejected candidate's system
    is not the kept one's); the cost is the branch case's to choose"""

    def __init__(self, n, seed):
        rng = np.random.default_rng(seed)
        J = rng.normal(size=(20, n))
        self.H, self.g = J.T @ J, rng.uniform(1.0, 2.0, n) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)

    def sums(self, two_d, k, cost, count=1000):
        return pack(two_d, cost, self.g * (1.0 + 0.125 * k), self.H * (1.0 + 0.0625 * k), count)


class Case:
    def __init__(self, name, two_d, max_iter, min_matches, x0, ref, sums, check):
        self.name, self.two_d, self.max_iter, self.min_matches, self.x0 = name, two_d, max_iter, min_matches, np.array(x0, F)
        self.ref, self.sums, self.check = ref, np.array(sums, F), check

    @property
    def script(self):
        return (self.two_d, self.max_iter, self.min_matches, self.x0, self.sums)


def drive(name, two_d, x0, source, check, max_iter=15, min_matches=0, limit=64):
    """runs the reference on source(ref, k, point) -> sums until it stops; check(ref) asserts the branch was reached"""
    ref = Reference(two_d, max_iter, min_matches, x0)
    sums, point = [], np.array(x0, F)
    while ref.code == NONE:
        assert len(sums) < limit, f"{name}: no stop within {limit} evaluations"
        s = source(ref, len(sums), point)
        sums.append(s)
        ref.feed(s)
        point = None if ref.candidate is None else np.array(ref.candidate, F)
    return Case(name, two_d, max_iter, min_matches, x0, ref, sums, check)


def decisions(ref):
    return "".join({"start": "S", "accept": "A", "reject": "R", "stop": "."}[t["decision"]] for t in ref.trace)


def by_rho(problem, two_d, rhos, first_cost=10.0, default=0.75):
    """a source: the cost of evaluation k >= 1 is the one that makes relative_decrease about rhos[k - 1]"""
    def source(ref, k, point):
        if k == 0:
            return problem.sums(two_d, 0, first_cost)
        rho = rhos[k - 1] if k - 1 < len(rhos) else default
        with np.errstate(all="ignore"):
            return problem.sums(two_d, k, ref.cost - F(rho) * ref.model_cost_change)
    return source


def expect(code, also=None):
    """a case's check: the way of ending, and `also` -- a condition (its value is asserted) or a function that asserts itself"""
    def check(ref):
        assert ref.code == code, (CODE_NAMES[ref.code], decisions(ref))
        if also:
            held = also(ref)
            assert held is None or held, (decisions(ref), [t["invalid"] for t in ref.trace])
    return check


# ---------------------------------------------------------------------------------------------------------------------
# the cases

INDEFINITE_SHRINKS = {1: 1.5e-4, 2: 4e-4, 3: 2e-3, 4: 2e-2}  # 1 / radius between the last radius that fails and the first that passes


def indefinite(n, inverse_radius):
    """H with a unit diagonal whose scaled, damped matrix Hs + D / radius (Hs_aa = D_a = 1/4) is positive definite only for
    1 / radius > inverse_radius: the off-diagonal entry (0, 1) is 1 + inverse_radius"""
    H = np.eye(n)
    H[0, 1] = H[1, 0] = 1.0 + inverse_radius
    return H


def _radius_after(shrinks, start=INITIAL_TRUST_REGION_RADIUS):
    r, f = F(start), F(2)
    for _ in range(shrinks):
        r, f = r / f, f * 2
    return r


def _cases_for(two_d):
    n = 3 if two_d else 6
    tag = "2d" if two_d else "3d"
    out = []

    def add(name, x0_active, source, check, **kw):
        out.append(drive(f"{tag}_{name}", two_d, start_point(two_d, x0_active), source, check, **kw))

    ones = np.ones(n)
    quad = Quadratic(n, 11, np.linspace(0.3, -0.4, n), floor=2.5)
    exact = Quadratic(n, 12, np.linspace(-0.2, 0.5, n))
    problem = lambda p: (lambda ref, k, point: p.sums(two_d, point))  # noqa: E731

    # ---- plain convergence
    add("quadratic_function_tolerance", np.linspace(1.0, 2.0, n), problem(quad), expect(FUNCTION, lambda r: decisions(r).startswith("SA")))
    add("quadratic_parameter_tolerance", np.linspace(1.0, 2.0, n) * 1e-3, problem(exact), expect(PARAMETER, lambda r: decisions(r).startswith("SA")))
    turned = np.linspace(1.0, 2.0, n)
    turned[-1] = 0.25 + 10000 * 2.0 * np.pi  # the yaw, 10000 turns: |x| is what the parameter tolerance compares the step with
    far = Quadratic(n, 13, np.concatenate([np.linspace(-0.2, 0.5, n - 1), [0.2 + 10000 * 2.0 * np.pi]]))
    add("quadratic_parameter_tolerance_turned", turned, problem(far), expect(PARAMETER, lambda r: r.x_norm > 6e4 and decisions(r).startswith("SA")))

    # ---- rejections
    def in_a_row(r):
        # (how the walk ends is the problem's business: by a tolerance, not by max_iter)
        assert "RRR" in decisions(r) and "RAR" in decisions(r) and decisions(r).count("A") >= 5 and r.code in (GRADIENT, PARAMETER, FUNCTION), decisions(r)
    valley_start = np.concatenate([[-1.2, 1.0], np.linspace(0.5, -0.5, n - 2)])
    add("valley", valley_start, problem(Valley()), in_a_row, max_iter=50)
    for mi in (0, 1, 2):
        add(f"valley_max_iter{mi}", valley_start, problem(Valley()), expect(MAX_ITERATIONS, lambda r, mi=mi: r.iteration == mi and len(r.trace) == mi + 1), max_iter=mi)
        add(f"quadratic_max_iter{mi}", np.linspace(1.0, 2.0, n) * 1e-3, problem(exact), expect(MAX_ITERATIONS, lambda r, mi=mi: r.iteration == mi), max_iter=mi)
    slope = Slope(n, 21)
    for order, rhos in (("ARRA", [0.75, -0.5, -2.0, 0.75]), ("RARA", [-0.5, 0.75, -1.0, 0.25]), ("RRAR", [-0.5, 0.0005, 1.0, -0.5]),
                        ("AARRRA", [0.25, 2.0, -0.5, -0.5, -0.5, 0.002])):
        add(f"orders_{order}", ones * 0.5, by_rho(slope, two_d, rhos), expect(MAX_ITERATIONS, lambda r, order=order: decisions(r) == "S" + order),
            max_iter=len(order))

    # ---- gradient tolerance
    def no_gradient(ref, k, point):
        return pack(two_d, 3.0, np.zeros(n), quad.H)
    add("gradient_zero_at_start", ones, no_gradient, expect(GRADIENT0, lambda r: len(r.trace) == 1))
    add("gradient_at_tolerance_at_start", ones, lambda ref, k, point: pack(two_d, 3.0, ones * GRADIENT_TOLERANCE, quad.H), expect(GRADIENT0))

    def gradient_later(ref, k, point):
        if k == 0:
            return slope.sums(two_d, 0, 1000.0)
        return pack(two_d, ref.cost - F(0.75) * ref.model_cost_change, ones * 1e-11 * (-1.0) ** k, slope.H)
    add("gradient_under_tolerance_later", ones, gradient_later, expect(GRADIENT, lambda r: decisions(r) == "SA" and r.iteration == 1))

    # ---- too few matches
    add("too_few_matches", ones, lambda ref, k, point: quad.sums(two_d, point, count=99), expect(NOT_ENOUGH_MATCHES, lambda r: r.skipped), min_matches=100)
    add("just_enough_matches", ones, lambda ref, k, point: quad.sums(two_d, point, count=100), expect(FUNCTION, lambda r: not r.skipped and r.matches == 100),
        min_matches=100)

    # ---- the invalid step: the factorization fails
    def failing(H_by_k, rho=0.5):
        def source(ref, k, point):
            H = H_by_k[min(k, len(H_by_k) - 1)]
            if k == 0:
                return pack(two_d, 1000.0, slope.g, H)
            return pack(two_d, ref.cost - F(rho) * ref.model_cost_change, slope.g * (1.0 + 0.125 * k), H)
        return source

    for shrinks, inv_r in INDEFINITE_SHRINKS.items():
        def reached(r, shrinks=shrinks):
            t = r.trace[0]
            assert t["invalid"] == shrinks and t["radii_tried"] == [_radius_after(i) for i in range(shrinks + 1)], t
            assert r.trace[0]["consecutive_invalid"] == 0 and r.unsuccessful == shrinks and r.iteration == shrinks + 1
        add(f"indefinite_passes_after_{shrinks}", ones, failing([indefinite(n, inv_r)]), expect(MAX_ITERATIONS, reached), max_iter=shrinks + 1)
    add("indefinite_fails_5_times", ones, failing([indefinite(n, 1.0)]),
        expect(INVALID_STEPS, lambda r: r.trace[0]["invalid"] == 5 and r.invalid == 5 and r.radius == _radius_after(4) and len(r.trace) == 1))

    def reset_reached(r):
        # 4 invalid steps, a valid one that is accepted at relative_decrease 1/2 (the radius stays), 4 invalid steps again
        assert [t["invalid"] for t in r.trace] == [4, 4, 0] and decisions(r) == "SAA", (decisions(r), r.trace)
        assert r.trace[1]["radii_tried"] == [_radius_after(i, _radius_after(4)) for i in range(5)]
        assert r.unsuccessful == 8 and r.successful == 3 and r.iteration == 10
    second = 0.5 * (1.0 / _radius_after(3, _radius_after(4)) + 1.0 / _radius_after(4, _radius_after(4)))
    add("invalid_4_valid_invalid_4", ones, failing([indefinite(n, INDEFINITE_SHRINKS[4]), indefinite(n, second)]), expect(MAX_ITERATIONS, reset_reached), max_iter=10)

    # ---- the invalid step: bad inputs
    def bad_at_start(change):
        def source(ref, k, point):
            s = quad.sums(two_d, point)
            change(s)
            return s
        return source

    act = ACTIVE_2D if two_d else ACTIVE_3D
    first, second_p, last = act[0], act[1], act[-1]

    def put(index, value):
        def change(s):
            s[index] = value
        return change
    five_invalid = expect(INVALID_STEPS, lambda r: r.trace[0]["invalid"] == 5 and len(r.trace) == 1 and r.iteration == 5)
    add("negative_diagonal", ones, bad_at_start(put(hidx(second_p, second_p), -1.0)), expect(INVALID_STEPS, lambda r: np.isnan(r.scale[1]) and r.trace[0]["invalid"] == 5))
    add("inf_diagonal", ones, bad_at_start(put(hidx(first, first), np.inf)), five_invalid)
    add("inf_off_diagonal", ones, bad_at_start(put(hidx(first, last), np.inf)), five_invalid)
    add("nan_off_diagonal", ones, bad_at_start(put(hidx(second_p, last), np.nan)), five_invalid)
    add("inf_gradient", ones, bad_at_start(put(1 + second_p, -np.inf)), five_invalid)
    add("nan_gradient_first", ones, bad_at_start(put(1 + first, np.nan)), five_invalid)
    add("nan_gradient_last", ones, bad_at_start(put(1 + last, np.nan)), five_invalid)

    def nan_gradient_small_rest(ref, k, point):
        g = ones * 1e-12
        g[1] = np.nan
        return pack(two_d, 3.0, g, quad.H)
    add("nan_gradient_rest_under_tolerance", ones, nan_gradient_small_rest, five_invalid)

    def bad_cost_at_candidate(value):
        def source(ref, k, point):
            s = quad.sums(two_d, point)
            if k == 1:
                s[0] = value
            return s
        return source
    for label, value in (("nan", np.nan), ("inf", np.inf)):
        add(f"{label}_cost_is_rejected", np.linspace(1.0, 2.0, n), bad_cost_at_candidate(value),
            expect(FUNCTION, lambda r: decisions(r).startswith("SRA") and r.unsuccessful == 1))

    def nan_cost_at_start(ref, k, point):
        s = quad.sums(two_d, point)
        if k == 0:
            s[0] = np.nan
        return s
    add("nan_cost_at_start", np.linspace(1.0, 2.0, n), nan_cost_at_start, expect(MAX_ITERATIONS, lambda r: decisions(r) == "SRRRR"), max_iter=4)

    def nan_gradient_accepted(ref, k, point):
        s = quad.sums(two_d, point)
        if k == 1:
            s[1 + last] = np.nan
        return s
    add("nan_gradient_of_an_accepted_point", np.linspace(1.0, 2.0, n), nan_gradient_accepted,
        expect(INVALID_STEPS, lambda r: decisions(r) == "SA" and r.trace[1]["invalid"] == 5 and np.isnan(r.result()[8 + 1 + last])))

    def overflow(ref, k, point):
        return pack(two_d, 1.0 if k == 0 else 0.5, ones * 1e200, np.eye(n) * 1e-12)
    add("model_cost_change_overflows", ones, overflow, expect(MAX_ITERATIONS, lambda r: decisions(r) == "SRRR" and np.isnan(r.model_cost_change)), max_iter=3)

    # ---- radius limits
    def uphill(ref, k, point):
        return pack(two_d, 1e60 * 2.0 ** k, ones * 1e30, np.eye(n))

    def min_radius_reached(r):
        assert decisions(r) == "S" + "R" * 15 and r.radius == F(1e4) * F(2.0) ** -120 and r.radius < MIN_TRUST_REGION_RADIUS
        assert r.trace[-2]["radius"] >= MIN_TRUST_REGION_RADIUS
    add("min_radius", np.zeros(n), uphill, expect(MIN_RADIUS, min_radius_reached), max_iter=40)

    def max_radius_reached(r):
        clamped = [t for t in r.trace if t.get("unclamped_radius", 0) > MAX_TRUST_REGION_RADIUS]
        assert clamped and all(t["radius"] == MAX_TRUST_REGION_RADIUS for t in clamped) and r.radius == MAX_TRUST_REGION_RADIUS
        assert decisions(r) == "S" + "A" * 28 and r.trace[-3]["radii_tried"] == [F(MAX_TRUST_REGION_RADIUS)]
    flat = Slope(n, 22)
    add("max_radius", ones * 0.5, lambda ref, k, point: pack(two_d, 1e3 if k == 0 else ref.cost - ref.model_cost_change, flat.g, flat.H),
        expect(MAX_ITERATIONS, max_radius_reached), max_iter=28)

    # ---- the lower clamp of the LM diagonal
    tiny = Quadratic(n, 14, np.linspace(0.3, -0.4, n), floor=2.5, column_scales=[1e-5] + [1.0] * (n - 1))
    add("min_diagonal", np.linspace(1.0, 2.0, n), problem(tiny),
        expect(FUNCTION, lambda r: r.trace[0].get("clamped_low") == [0] and r.trace[0]["diag"][0] == MIN_LM_DIAGONAL and "clamped_high" not in r.trace[0]))

    # ---- the acceptance threshold
    for label, (cost0, cost1, rho) in _threshold_costs(two_d, slope).items():
        def source(ref, k, point, cost0=cost0, cost1=cost1):
            if k <= 1:
                return slope.sums(two_d, k, cost0 if k == 0 else cost1)
            return slope.sums(two_d, k, ref.cost - F(0.75) * ref.model_cost_change)
        want = "SAA" if label == "above" else "SRA"

        def at_threshold(r, rho=rho, label=label, want=want):
            got = r.trace[1]["relative_decrease"]
            assert got == rho and decisions(r) == want, (got, rho, decisions(r))
            assert {"above": got > MIN_RELATIVE_DECREASE, "below": got < MIN_RELATIVE_DECREASE, "equal": got == MIN_RELATIVE_DECREASE}[label]
        add(f"threshold_{label}", ones * 0.5, source, expect(MAX_ITERATIONS, at_threshold), max_iter=2)
    return out


def _threshold_costs(two_d, slope):
    """{above | below | equal: (cost at the start, cost at the first candidate, relative_decrease)}: `above` and `below`
    and `below` are the two representable costs on either side of min_relative_decrease that are nearest to each other: adjacent, or with the
    costs that hit it exactly (`equal`: the first of them) between them.  The start cost is
    twice the cost change wanted, so the change is exact (Sterbenz) and walks through every value near it."""
    probe = Reference(two_d, 2, 0, start_point(two_d, np.ones(3 if two_d else 6) * 0.5))
    probe.feed(slope.sums(two_d, 0, 1.0))
    m = probe.model_cost_change  # (does not depend on the cost)
    cost0 = F(2e-3) * m
    with np.errstate(all="ignore"):
        rho = lambda c: (cost0 - c) / m  # noqa: E731
        c = cost0 - F(1e-3) * m
        while rho(c) > MIN_RELATIVE_DECREASE:
            c = np.nextafter(c, F(np.inf))
        while not rho(c) > MIN_RELATIVE_DECREASE:
            c = np.nextafter(c, F(-np.inf))
        # c: the largest cost that is accepted
        above, after = c, np.nextafter(c, F(np.inf))
        out = {"above": (cost0, above, rho(above))}
        # the costs behind it: those that hit the threshold exactly (rejected: the rule is `>`), then the first under it
        equal = []
        while rho(after) == MIN_RELATIVE_DECREASE:
            equal.append(after)
            after = np.nextafter(after, F(np.inf))
        assert rho(after) < MIN_RELATIVE_DECREASE
        if equal:
            out["equal"] = (cost0, equal[0], rho(equal[0]))
        out["below"] = (cost0, after, rho(after))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """every case, 3D then 2D, built once per process and left unchanged"""
    return tuple(_cases_for(False) + _cases_for(True))


def canonical(a):
    """bit patterns with every NaN made the same one (as tests/test_gpu_numerics.py compares)"""
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def compare(cases_, records, results, status):
    """failure strings of (records, results, status) as lidarslam_amd.selftest_lm_step returns them against the reference"""
    fails = []
    for c, rec, res, st in zip(cases_, records, results, status):
        want = np.array(c.ref.records)
        if tuple(st) != (0, len(want)):
            fails.append(f"{c.name}: status {tuple(st)}, the reference stops after {len(want)} evaluations")
            continue
        bad = np.argwhere(canonical(rec) != canonical(want))
        if bad.size:
            k, i = bad[0]
            fails.append(f"{c.name}: {len(bad)} record entries differ, first at evaluation {k} entry {i}: {rec[k, i]!r}, reference {want[k, i]!r}"
                         f" (reference: {decisions(c.ref)}, {CODE_NAMES[c.ref.code]}; got code {int(rec[len(want) - 1, 6])})")
        bad = np.flatnonzero(canonical(res) != canonical(c.ref.result()))
        if bad.size:
            fails.append(f"{c.name}: result entries {bad.tolist()} differ: {res[bad[:4]].tolist()}, reference {c.ref.result()[bad[:4]].tolist()}")
    return fails
