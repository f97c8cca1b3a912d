// lsa_lm.h -- LidarSlam::LocalOptimizer for the MI355X path
// (slam_lib/include/LidarSlam/LocalOptimizer.h, slam_lib/src/LocalOptimizer.cxx).
//
// The residual blocks live on the device (lsa_match wrote them); every evaluation the
// trust-region loop asks for is one lsa_accumulate call (cost, gradient, J^T J reduced on
// the GPU, 29 doubles read back).  The 6-dof Levenberg-Marquardt control flow of Ceres
// (unpinned master >= 2.0 in the reference CI) is restated on the host: Jacobi scaling,
// LM diagonal, step acceptance, radius update, termination tests.
#pragma once
#include <array>
#include "../lsa_ctx.h"
#include "lsa_hostmath.h"
#include "lsa_lm_loop.h"  // SolveSummary, the loop itself

namespace lsa
{
namespace host
{

// LocalOptimizer::RegistrationError (LocalOptimizer.h:36-52)
struct RegistrationError
{
  double PositionError = 0.;
  double PositionErrorDirection[3] = {0, 0, 0};
  double OrientationError = 0.;
  double OrientationErrorDirection[3] = {0, 0, 0};
  std::array<double, 36> Covariance{};
};

class LocalOptimizer
{
public:
  explicit LocalOptimizer(lsa_ctx* ctx) : Ctx(ctx) {}
  void SetTwoDMode(bool b) { TwoDMode = b; }
  void SetLMMaxIter(unsigned n) { LMMaxIter = n; }
  void SetPosePrior(const Pose& prior) { ToXYZRPY(prior, PoseArray); HaveFinal = false; }
  // residual blocks = the device records of the last lsa_match of every type in the mask
  void UseDeviceResiduals(unsigned typeMask) { TypeMask = typeMask; }
  // Slam.cxx:919-923 / 1098-1107 skip the optimisation when too few keypoints matched.  The count comes
  // back with the first evaluation, so the caller does not have to read the match histograms first.
  void SetMinMatches(unsigned n) { MinMatches = n; }
  // the trust-region loop on the device, one launch per solve (lsa_solve_device); when off, or when the device gives
  // up, the loop runs here with one launch per evaluation.  Same decisions from the same sums either way.
  void SetDeviceLoop(bool b) { DeviceLoop = b; }
  int Solve(SolveSummary& summary);
  // The second half of a solve enqueued with lsa_solve_device_begin[_linked] (device loop only): waits for the result of the
  // oldest solve begun on this context; SetPosePrior must have been called with the pose that solve starts from.  A device
  // solve that gave up is redone on the host -- End then returns 1: the iterations enqueued ahead have been called off.
  int End(SolveSummary& summary);
  Pose GetOptimizedPose() const { return FromXYZRPY(PoseArray); }
  int EstimateRegistrationError(RegistrationError& err);

private:
  lsa_ctx* Ctx;
  unsigned TypeMask = 7;
  bool TwoDMode = false;
  unsigned LMMaxIter = 15;
  unsigned MinMatches = 0;
  double PoseArray[6] = {0, 0, 0, 0, 0, 0};
  bool DeviceLoop = true;
  // normal equations at PoseArray as the device solve returned them (EstimateRegistrationError needs no evaluation then)
  bool HaveFinal = false;
  double FinalH[36];
  int SolveOnHost(SolveSummary& summary);
  void TakeResult(const lsa_solve_result_t& r, SolveSummary& summary);
};

// SolveSPD (lsa_lm_loop.cpp) / SymEigen for the self-test (lsa_selftest_numerics)
bool ProbeSolveSPD(int n, const double* A, const double* b, double* x);
void ProbeSymEigen(int n, const double* A, double* evals, double* evecs);

}  // namespace host
}  // namespace lsa
