// lsa_lm.cpp -- see lsa_lm.h.  Solver options: slam_lib/src/LocalOptimizer.cxx:93-96
// (DENSE_QR, max_num_iterations = LMMaxIter, everything else Ceres defaults).
#include "lsa_sym_eigen.h"
#include "lsa_lm.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace lsa
{
namespace host
{
// lsa_selftest_numerics, fn 8-11: the loop's solver (lsa_lm_loop.cpp) and the eigen-solver on one record (layouts: include/lidarslam_amd.h)
bool ProbeSolveSPD(int n, const double* A, const double* b, double* x) { return SolveSPD(n, A, b, x); }
void ProbeSymEigen(int n, const double* A, double* evals, double* evecs) { SymEigen(n, A, evals, evecs); }

void LocalOptimizer::TakeResult(const lsa_solve_result_t& r, SolveSummary& sum)
{
  sum = SolveSummary();
  sum.num_successful_steps = r.num_successful_steps;
  sum.num_unsuccessful_steps = r.num_unsuccessful_steps;
  sum.num_iterations = r.num_iterations;
  sum.num_evaluations = r.num_evaluations;
  sum.initial_cost = r.initial_cost;
  sum.final_cost = r.final_cost;
  sum.num_matches = r.num_matches;
  sum.skipped = r.skipped != 0;
  sum.message = r.message;
  if (!sum.skipped)
  {
    std::memcpy(PoseArray, r.pose, sizeof(PoseArray));
    std::memcpy(FinalH, r.H, sizeof(FinalH));
    HaveFinal = true;
  }
}

int LocalOptimizer::Solve(SolveSummary& sum)
{
  HaveFinal = false;
  if (DeviceLoop)
  {
    lsa_solve_result_t r;
    const int rc = lsa_solve_device(Ctx, TypeMask, PoseArray, TwoDMode ? 1 : 0, static_cast<int>(LMMaxIter), static_cast<int>(MinMatches), &r);
    if (rc == LSA_OK)
    {
      TakeResult(r, sum);
      return LSA_OK;
    }
    if (rc != LSA_E_STATE) return rc;  // LSA_E_STATE: the device gave up, nothing was changed
  }
  return SolveOnHost(sum);
}

int LocalOptimizer::End(SolveSummary& sum)
{
  HaveFinal = false;
  lsa_solve_result_t r;
  const int rc = lsa_solve_device_end(Ctx, &r);
  if (lsa_icp_trace_on()) std::fprintf(stderr, "[optimizer end] rc %d (%s)\n", rc, rc ? lsa_last_error(Ctx) : "");
  if (rc == LSA_OK)
  {
    TakeResult(r, sum);
    return LSA_OK;
  }
  if (rc != LSA_E_STATE) return rc;
  // the solve gave up: the residual blocks are there, the loop runs here.  Whatever was enqueued ahead has been called off
  // (lsa_solve_device_end): 1 tells the caller
  const int hrc = SolveOnHost(sum);
  return hrc < 0 ? hrc : 1;
}

int LocalOptimizer::SolveOnHost(SolveSummary& sum)
{
  int act[6], n = 0;
  for (int i = 0; i < 6; ++i)
    if (!(TwoDMode && (i == 2 || i == 3 || i == 4))) act[n++] = i;  // SubsetParameterization(6, {2,3,4}), LocalOptimizer.cxx:89-90
  // the loop is lsa_lm_loop.cpp's; every evaluation it asks for is one lsa_accumulate call
  const LmEvaluate evaluate = [&](const double* w, LmEval& e) -> int { return lsa_accumulate(Ctx, TypeMask, w, 1, &e.cost, e.g, e.H, &e.nValid); };
  return RunLmLoop(act, n, PoseArray, static_cast<int>(LMMaxIter), MinMatches, evaluate, sum, nullptr, nullptr, nullptr);
}

// LocalOptimizer.cxx:112-140: covariance = pseudo-inverse of the loss-corrected J^T J
// (DENSE_SVD, null_space_rank -1 => singular value ratios below sqrt(1e-14) are dropped)
int LocalOptimizer::EstimateRegistrationError(RegistrationError& err)
{
  err = RegistrationError();
  int act[6], n = 0;
  for (int i = 0; i < 6; ++i)
    if (!(TwoDMode && (i == 2 || i == 3 || i == 4))) act[n++] = i;
  LmEval cur;
  if (HaveFinal) std::memcpy(cur.H, FinalH, sizeof(FinalH));
  else
  {
    const int rc = lsa_accumulate(Ctx, TypeMask, PoseArray, 1, &cur.cost, cur.g, cur.H, &cur.nValid);
    if (rc) return rc;
  }
  double H[36], evals[6], evecs[36];
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) H[a * n + b] = cur.H[act[a] * 6 + act[b]];
  SymEigen(n, H, evals, evecs);
  const double lmax = evals[n - 1];
  double inv[6];
  bool truncated = false;
  for (int i = n - 1; i >= 0; --i)
  {
    const double ratio = lmax > 0 ? std::sqrt(std::max(evals[i], 0.0) / lmax) : 0.0;
    if (truncated || ratio < std::sqrt(1e-14)) { truncated = true; inv[i] = 0.0; }
    else inv[i] = 1.0 / evals[i];
  }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
    {
      double s = 0;
      for (int k = 0; k < n; ++k) s += evecs[a * n + k] * inv[k] * evecs[b * n + k];
      err.Covariance[act[a] * 6 + act[b]] = s;
    }
  auto block = [&](int o, double& e, double* dir) {
    double B[9], ev[3], vec[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) B[i * 3 + j] = err.Covariance[(o + i) * 6 + (o + j)];
    SymEigen(3, B, ev, vec);
    e = std::sqrt(ev[2]);
    for (int i = 0; i < 3; ++i) dir[i] = vec[i * 3 + 2];
  };
  block(0, err.PositionError, err.PositionErrorDirection);
  block(3, err.OrientationError, err.OrientationErrorDirection);
  err.OrientationError = err.OrientationError / M_PI * 180.;
  return LSA_OK;
}

}  // namespace host
}  // namespace lsa
