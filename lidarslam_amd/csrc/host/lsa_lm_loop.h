// lsa_lm_loop.h -- the trust-region loop of LocalOptimizer::Solve with the evaluation as a callback: the 6-dof
// Levenberg-Marquardt control flow of Ceres (Jacobi scaling, LM diagonal, damped Cholesky solve, step acceptance, radius
// update, termination tests) on 29 sums per evaluation, whoever works them out -- lsa_accumulate on a device
// (LocalOptimizer::SolveOnHost) or a script (lsa_selftest_lm_host).  No device headers: a stand-alone program compiles
// lsa_lm_loop.cpp by itself.
#pragma once
#include <functional>

namespace lsa
{
namespace host
{

// counterpart of ceres::Solver::Summary fields the reference reads (Slam.cxx:950, 1151)
struct SolveSummary
{
  int num_successful_steps = 0;
  int num_unsuccessful_steps = 0;
  int num_iterations = 0;
  int num_evaluations = 0;
  double initial_cost = 0., final_cost = 0.;
  int num_matches = 0;      // residual blocks (successful matches) the problem was built from
  bool skipped = false;     // fewer than SetMinMatches(): nothing was optimised, the prior is returned
  const char* message = "";
};

// one evaluation: cost, gradient, J^T J (6 x 6, row-major, both triangles) and the number of residual blocks
struct LmEval
{
  double cost = 0.;
  double g[6] = {0};
  double H[36] = {0};
  int nValid = 0;
};

// how a solve ended: the codes of lsa_solve_result_t::termination (lsa_lm.hip: LmCode)
enum LmTermination
{
  kLmNone = 0, kLmNotEnoughMatches, kLmGradient0, kLmMaxIterations, kLmGradient, kLmMinRadius, kLmInvalidSteps, kLmParameterTolerance,
  kLmFunctionTolerance
};
const char* LmMessage(int termination);

// One record per evaluation, written when the loop has decided what to do with it (include/lidarslam_amd.h,
// lsa_selftest_lm_step: the device's step writes the same record).
constexpr int kLmRecordDoubles = 42;
constexpr int kLmResultDoubles = 45;
struct LmTrace
{
  double* records = nullptr;  // [capacity][kLmRecordDoubles]
  int capacity = 0;
  int count = 0;              // evaluations decided on (may exceed capacity: the records beyond it are not written)
};

// evaluate(w, e): the sums at w; not 0 ends the loop, which returns that value and leaves x alone.
typedef std::function<int(const double* w, LmEval& e)> LmEvaluate;

// The loop.  act[n]: the active parameters (all 6, or x y rz in 2D mode); x: the start point, the solve's pose afterwards;
// termination: how it ended; last: the sums at the final point (all 0 when the solve was skipped); trace: may be null.
int RunLmLoop(const int* act, int n, double x[6], int max_iter, unsigned min_matches, const LmEvaluate& evaluate, SolveSummary& sum, int* termination,
              LmEval* last, LmTrace* trace);

// small dense symmetric positive definite solve (normal equations of the augmented LM system)
bool SolveSPD(int n, const double* A, const double* b, double* x);

}  // namespace host
}  // namespace lsa
