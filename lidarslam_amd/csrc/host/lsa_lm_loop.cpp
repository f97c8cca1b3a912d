// lsa_lm_loop.cpp -- see lsa_lm_loop.h.  Solver options: slam_lib/src/LocalOptimizer.cxx:93-96
// (DENSE_QR, max_num_iterations = LMMaxIter, everything else Ceres defaults).
#include "lsa_lm_loop.h"
#include "../../../include/lidarslam_amd.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace lsa
{
namespace host
{

bool SolveSPD(int n, const double* A, const double* b, double* x)
{
  // (divisions by a diagonal element are multiplications by its reciprocal, taken once: as solve_spd of lsa_lm.hip)
  double L[36], rinv[6];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j)
    {
      double s = A[i * n + j];
      for (int k = 0; k < j; ++k) s -= L[i * n + k] * L[j * n + k];
      if (i == j)
      {
        if (!(s > 0.0) || !std::isfinite(s)) return false;
        L[i * n + i] = std::sqrt(s);
        rinv[i] = 1.0 / L[i * n + i];
      }
      else
        L[i * n + j] = s * rinv[j];
    }
  double y[6];
  for (int i = 0; i < n; ++i)
  {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= L[i * n + k] * y[k];
    y[i] = s * rinv[i];
  }
  for (int i = n - 1; i >= 0; --i)
  {
    double s = y[i];
    for (int k = i + 1; k < n; ++k) s -= L[k * n + i] * x[k];
    x[i] = s * rinv[i];
  }
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

const char* LmMessage(int termination)
{
  static const char* const kMessages[] = {"", "not enough matches", "gradient tolerance (iteration 0)", "max iterations", "gradient tolerance",
                                          "min trust region radius", "too many invalid steps", "parameter tolerance", "function tolerance"};
  return kMessages[std::min(std::max(termination, 0), 8)];
}

int RunLmLoop(const int* act, int n, double x[6], int max_iter, unsigned min_matches, const LmEvaluate& evaluate_sums, SolveSummary& sum, int* termination,
              LmEval* last, LmTrace* trace)
{
  sum = SolveSummary();
  if (last) *last = LmEval();
  if (termination) *termination = kLmNone;

  // ceres::Solver::Options defaults
  const double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  const double min_relative_decrease = 1e-3, min_trust_region_radius = 1e-32, max_radius = 1e16;
  const double min_diagonal = 1e-6, max_diagonal = 1e32;
  const int max_consecutive_invalid = 5;
  double radius = 1e4, decrease_factor = 2.0;
  bool reuse_diagonal = false;

  auto evaluate = [&](const double* w, LmEval& e) -> int {
    sum.num_evaluations++;
    return evaluate_sums(w, e);
  };

  // what the record shows beside the summary (the device's step keeps the same between two evaluations)
  double scale[6] = {1, 1, 1, 1, 1, 1}, diag[6] = {0};
  double x_norm = 0., model_cost_change = 0., delta_norm = 0.;
  int consecutive_invalid = 0, iter = 0;
  int adopted = 0;  // evaluations whose sums became the current ones: the start point's and every accepted candidate's
  // the record of the evaluation just decided on: with the next candidate, or with the way the solve ended
  auto record = [&](const double* cand, int code) {
    if (termination) *termination = code;
    sum.message = LmMessage(code);
    if (!trace) return;
    const int k = trace->count++;
    if (k >= trace->capacity) return;
    double* o = trace->records + (size_t)k * kLmRecordDoubles;
    for (int a = 0; a < 6; ++a) o[a] = cand ? cand[a] : 0.;
    o[6] = code;
    o[7] = cand ? 0. : 1.;
    o[8] = radius; o[9] = decrease_factor; o[10] = x_norm; o[11] = model_cost_change; o[12] = delta_norm; o[13] = sum.initial_cost;
    o[14] = reuse_diagonal ? 1. : 0.;
    o[15] = consecutive_invalid;
    o[16] = iter;
    o[17] = sum.num_evaluations + (cand ? 1 : 0);  // with the candidate's, which is under way on the device when it writes this
    o[18] = sum.num_successful_steps; o[19] = sum.num_unsuccessful_steps; o[20] = sum.num_iterations;
    o[21] = sum.skipped ? 1. : 0.;
    o[22] = sum.num_matches;
    for (int a = 0; a < 6; ++a) { o[23 + a] = x[a]; o[29 + a] = scale[a]; o[35 + a] = diag[a]; }
    o[41] = adopted & 1;
  };

  double start[6];
  std::memcpy(start, x, sizeof(start));
  LmEval cur;
  int rc = evaluate(x, cur);
  if (rc) return rc;
  sum.num_matches = cur.nValid;
  if (static_cast<unsigned>(cur.nValid) < min_matches)
  {
    sum.skipped = true;
    record(nullptr, kLmNotEnoughMatches);
    return LSA_OK;
  }
  sum.initial_cost = sum.final_cost = cur.cost;
  sum.num_successful_steps = 1;  // iteration 0 is reported as a successful step by Ceres
  adopted = 1;

  for (int a = 0; a < n; ++a) scale[a] = 1.0 / (1.0 + std::sqrt(cur.H[act[a] * 6 + act[a]]));  // Jacobi scaling, once
  // max |g_a| <= tolerance, entry by entry: a gradient with a NaN in it has not converged (std::max would drop the NaN)
  auto gradBelow = [&](const LmEval& e) {
    for (int a = 0; a < n; ++a)
      if (!(std::abs(e.g[act[a]]) <= gradient_tolerance)) return false;
    return true;
  };
  auto xnorm = [&](const double* v) { double s = 0; for (int a = 0; a < n; ++a) s += v[act[a]] * v[act[a]]; return std::sqrt(s); };

  if (gradBelow(cur))
  {
    record(nullptr, kLmGradient0);
    if (last) *last = cur;
    return LSA_OK;
  }
  x_norm = xnorm(x);

  while (true)
  {
    if (iter >= max_iter) { record(nullptr, kLmMaxIterations); break; }
    if (gradBelow(cur)) { record(nullptr, kLmGradient); break; }
    if (radius < min_trust_region_radius) { record(nullptr, kLmMinRadius); break; }
    ++iter;
    sum.num_iterations = iter;

    double Hs[36], gs[6];
    for (int a = 0; a < n; ++a)
    {
      gs[a] = cur.g[act[a]] * scale[a];
      for (int b = 0; b < n; ++b) Hs[a * n + b] = cur.H[act[a] * 6 + act[b]] * scale[a] * scale[b];
    }
    if (!reuse_diagonal)
      for (int a = 0; a < n; ++a) diag[a] = std::min(std::max(Hs[a * n + a], min_diagonal), max_diagonal);
    double M[36], y[6], step[6];
    for (int i = 0; i < n * n; ++i) M[i] = Hs[i];
    for (int a = 0; a < n; ++a) M[a * n + a] += diag[a] / radius;
    bool ok = SolveSPD(n, M, gs, y);
    reuse_diagonal = true;
    double change = 0;
    if (ok)
    {
      for (int a = 0; a < n; ++a) step[a] = -y[a];
      double sg = 0, sHs = 0;
      for (int a = 0; a < n; ++a)
      {
        sg += step[a] * gs[a];
        double t = 0;
        for (int b = 0; b < n; ++b) t += Hs[a * n + b] * step[b];
        sHs += step[a] * t;
      }
      change = -sg - 0.5 * sHs;
      if (change < 0.0) ok = false;
    }
    if (!ok)
    {
      ++sum.num_unsuccessful_steps;
      if (++consecutive_invalid >= max_consecutive_invalid) { record(nullptr, kLmInvalidSteps); break; }
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
      continue;
    }
    consecutive_invalid = 0;
    model_cost_change = change;

    double cand[6];
    delta_norm = 0;
    std::memcpy(cand, x, sizeof(cand));
    for (int a = 0; a < n; ++a)
    {
      cand[act[a]] = x[act[a]] + step[a] * scale[a];
      const double e = x[act[a]] - cand[act[a]];
      delta_norm += e * e;
    }
    delta_norm = std::sqrt(delta_norm);
    record(cand, kLmNone);
    // Ceres evaluates the cost only here and, if the step is accepted, residuals + Jacobian again at
    // the same point.  On the device the Jacobian costs nothing extra (the kernel is bound by the
    // record reads), so it is evaluated speculatively and reused on acceptance: one launch + one
    // read-back per LM iteration instead of two, same arithmetic.
    LmEval cc;
    rc = evaluate(cand, cc);
    if (rc)
    {
      std::memcpy(x, start, sizeof(start));
      return rc;
    }

    // parameter / function tolerance terminate WITHOUT taking the candidate step
    if (delta_norm <= parameter_tolerance * (x_norm + parameter_tolerance)) { record(nullptr, kLmParameterTolerance); break; }
    const double cost_change = cur.cost - cc.cost;
    if (std::abs(cost_change) <= function_tolerance * cur.cost) { record(nullptr, kLmFunctionTolerance); break; }

    const double relative_decrease = cost_change / model_cost_change;
    if (relative_decrease > min_relative_decrease)
    {
      std::memcpy(x, cand, sizeof(cand));
      x_norm = xnorm(x);
      cur = cc;  // gradient and J^T J at the accepted point were evaluated speculatively above
      ++adopted;
      ++sum.num_successful_steps;
      const double t = 2.0 * relative_decrease - 1.0;
      radius = std::min(max_radius, radius / std::max(1.0 / 3.0, 1.0 - t * t * t));
      decrease_factor = 2.0;
      reuse_diagonal = false;
    }
    else
    {
      ++sum.num_unsuccessful_steps;
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = true;
    }
  }
  sum.final_cost = cur.cost;
  if (last) *last = cur;
  return LSA_OK;
}

}  // namespace host
}  // namespace lsa

// lsa_selftest_lm_host (include/lidarslam_amd.h): the loop above on scripted sums, no device and no context
extern "C" int lsa_selftest_lm_host(int n_scripts, const int* header, const double* x0, const double* sums, double* records, double* results, int* status)
{
  using namespace lsa::host;
  if (n_scripts <= 0 || !header || !x0 || !sums || !records || !results || !status) return LSA_E_ARG;
  for (int s = 0; s < n_scripts; ++s)
    if (header[4 * s + 1] < 0 || header[4 * s + 3] < 1 || header[4 * s + 3] > 4096) return LSA_E_ARG;
  size_t first = 0;
  for (int s = 0; s < n_scripts; ++s)
  {
    const int two_d = header[4 * s], max_iter = header[4 * s + 1], min_matches = header[4 * s + 2], K = header[4 * s + 3];
    int act[6], n = 0;
    for (int i = 0; i < 6; ++i)
      if (!(two_d && (i == 2 || i == 3 || i == 4))) act[n++] = i;
    const double* script = sums + first * 29;
    int used = 0;
    const LmEvaluate evaluate = [&](const double*, LmEval& e) -> int {
      if (used >= K) return 1;  // the script ran out before the loop stopped
      const double* v = script + (size_t)used * 29;
      ++used;
      e.cost = v[0];
      for (int a = 0; a < 6; ++a) e.g[a] = v[1 + a];
      int h = 7;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) { e.H[a * 6 + b] = v[h]; e.H[b * 6 + a] = v[h]; ++h; }
      e.nValid = (int)v[28];
      return 0;
    };
    double* rec = records + first * kLmRecordDoubles;
    std::memset(rec, 0, (size_t)K * kLmRecordDoubles * sizeof(double));
    LmTrace trace;
    trace.records = rec;
    trace.capacity = K;
    double x[6];
    std::memcpy(x, x0 + (size_t)s * 6, sizeof(x));
    SolveSummary sum;
    LmEval last;
    int code = kLmNone;
    const int rc = RunLmLoop(act, n, x, max_iter, (unsigned)std::max(min_matches, 0), evaluate, sum, &code, &last, &trace);
    status[2 * s] = rc ? 1 : 0;
    status[2 * s + 1] = used;
    double* r = results + (size_t)s * kLmResultDoubles;
    std::memset(r, 0, kLmResultDoubles * sizeof(double));
    if (!rc)
    {
      // the layout of the device solve's result (lsa_lm.hip: kRes*)
      for (int a = 0; a < 6; ++a) r[a] = x[a];
      r[6] = sum.initial_cost;
      r[7] = last.cost;
      r[8] = last.cost;
      for (int a = 0; a < 6; ++a) r[9 + a] = last.g[a];
      int h = 15;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) r[h++] = last.H[a * 6 + b];
      r[36] = last.nValid;
      r[37] = sum.num_successful_steps; r[38] = sum.num_unsuccessful_steps; r[39] = sum.num_iterations; r[40] = sum.num_evaluations;
      r[41] = sum.skipped ? 1. : 0.;
      r[42] = code;
      r[43] = sum.num_matches;
    }
    first += (size_t)K;
  }
  return LSA_OK;
}
