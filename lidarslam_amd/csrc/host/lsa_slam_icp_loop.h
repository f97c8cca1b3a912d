// lsa_slam_icp_loop.h -- the one ICP loop driver of SlamCore, for the units that run a loop: ComputeEgoMotion() and
// Localization() (lsa_slam_icp.cpp), RegisterLoggedFrames() (lsa_slam_log.cpp).  A template in a header: every loop is
// instantiated with its caller's lambdas inlined.
#pragma once
#include <cstdio>
#include <cstdlib>
#include "lsa_slam_internal.h"

namespace lsa
{
namespace host
{
constexpr unsigned kChainMax = 6;  // ICP iterations of one loop enqueued at once behind links (lsa_icp_link: 7 blocks, 7 mailboxes)
#define ICP_TRACE(...) do { if (lsa_icp_trace_on()) std::fprintf(stderr, __VA_ARGS__); } while (0)

// ---- the ICP loop of ComputeEgoMotion() and Localization() ---------------------------------------------------------------
// What the two tell RunIcpLoop about their loop; what only one of them does at some point of an iteration is a callable.
struct SlamCore::IcpLoopSpec
{
  const char* name;                        // "ego" / "loc" / "reg" (trace lines)
  lsa_ctx* ctx;                            // the context the loop drives; NULL: the frame path's own
  bool inLine;                             // strictly in line whatever ICPAhead says
  int target, set;                         // the LSA_TARGET_* searched, the LSA_SET_* matched against it
  unsigned matchMask, solveMask;           // keypoint types matched / whose residual blocks the solves take
  unsigned maxIter, lmMaxIter;
  double initSaturation, finalSaturation;  // the saturation distance goes from one to the other over the loop
  lsa_match_params_t match;
  int loopBit;                             // this loop's bit of LSA_ICP_AHEAD_LOOPS
  bool linksOk;                            // this loop's iterations can wait behind links at all
  int undistortAhead;                      // `undistort` of lsa_match_types_linked: a search enqueued ahead starts with RefineUndistortion
  lsa_icp_link_t link;                     // what the loop's solves need to leave a link (`first` is the driver's)
  long long* matchSerial;                  // lsa_match_serial per type, of the iteration whose result was read last
  double FrameStats::*icpSeconds;          // stage timers: an iteration's enqueueing, the wait for its solve
  double FrameStats::*lmSeconds;
  int FrameStats::*iterations;
  bool countSkippedEvals;                  // Stats.lm_evals takes in the evaluation of a skipped solve
};
// A RefineUndistortion between two iterations that is not applied by a launch of its own
struct SlamCore::IcpUndistortion
{
  Pose d0 = Pose::Identity(), d1 = Pose::Identity();
  bool pending = false;  // the undistortion the last iteration ended with has not been applied yet
};

namespace
{
constexpr auto kNothing = [](auto&&...) { return LSA_OK; };  // the callable of a loop that does nothing at that point
// diagnostics, read once
const int kAheadLoops = std::getenv("LSA_ICP_AHEAD_LOOPS") ? std::atoi(std::getenv("LSA_ICP_AHEAD_LOOPS")) : 3;  // the loops that enqueue ahead at all: 1 ego-motion only, 2 localization only
}  // namespace

// How an ICP loop's iterations reach the device: the one place where that is written down.  `pose` is the pose the loop
// iterates (prior of every solve, replaced by every accepted result).  The callables, all returning an LSA_* code:
//   top(icpIter)                      before anything of the iteration is enqueued
//   enqueued(icpIter)                 between the iteration's enqueueing and the wait for its solve
//   solved()                          the solve's result is there
//   skipped()                         ... with too few matches: the loop ends
//   accepted(last, undistortion)      `pose` is the solve's; what was enqueued ahead has been called off if `last`.  A
//                                     RefineUndistortion left in `undistortion` (pending) rides in the next search
//   finished(optimizer)               after the last accepted iteration
// In line (ICPAhead = 0, spec.inLine, and the fall-back of the other): match, solve, and the next match once the pose is known.
// Links (any other ICPAhead): the WHOLE loop is enqueued at once, every solve leaving pose and start point for the iteration
// behind it on the device (lsa_icp_link) -- no host between two iterations, nothing spins; this thread reads the results as
// they arrive, takes the decisions the device has taken already and does its own pose algebra beside the running device.
// What cannot be linked -- a loop longer than kChainMax, !spec.linksOk, a match lsa_match_types_linked refuses -- runs in
// line from there on.
// (There is no third schedule with iteration i + 1 behind a gate kernel that polls host memory for the pose.  It was here
// once and gained nothing measurable over links (0.0985 against 0.0976 ms an iteration); with host maps and a second
// context alive a waiting gate once kept the device from delivering any result for two seconds, which was never
// explained.  It was removed rather than fenced off.)
template <class Top, class Enqueued, class Solved, class Skipped, class Accepted, class Finished>
int SlamCore::RunIcpLoop(const IcpLoopSpec& spec, Pose& pose, const Top& top, const Enqueued& enqueued, const Solved& solved, const Skipped& skipped,
                         const Accepted& accepted, const Finished& finished)
{
  lsa_ctx* const ctx = spec.ctx ? spec.ctx : Ctx;  // the context the loop drives
  const bool own = ctx == Ctx;                      // ... the frame path's: the look-ahead's interlude rides in its solves
  TotalMatchedKeypoints = 0;
  lsa_match_params_t mp = spec.match;
  auto saturation = [&](unsigned icpIter) {
    const double iterRatio = icpIter / static_cast<double>(spec.maxIter - 1);
    return (1 - iterRatio) * spec.initSaturation + iterRatio * spec.finalSaturation;
  };
  bool chain = !spec.inLine && ICPAhead != 0 && DeviceLM && FusedMatch && (kAheadLoops & spec.loopBit) && spec.maxIter <= kChainMax && spec.linksOk;
  if (chain) lsa_icp_abandon(ctx);
  unsigned chained = 0;            // iterations 0 .. chained - 1 are in the queue (links)
  long long chainSerial[kChainMax][3] = {};
  IcpUndistortion undistortion;
  unsigned icpIter = 0;

  // Every way out calls off what is still in the queue: the links' iterations when the loop ends in front of them (the
  // device has taken the same decision from the same result -- the iterations behind do nothing; what their matches
  // announced on the host is taken back).  After an error nobody will end the solves begun: all of it goes.
  auto callOffRest = [&](bool all) {
    if (all || icpIter + 1 < chained)
    {
      lsa_icp_abandon(ctx);
      chained = 0;
    }
  };
  struct AtExit { decltype(callOffRest)& callOffRest; bool failed; ~AtExit() { callOffRest(failed); } } atExit{callOffRest, true};

  auto takeSerials = [&](long long* serial) {
    for (int k = 0; k < 3; ++k)
      if ((spec.matchMask >> k) & 1u) serial[k] = lsa_match_serial(ctx, k);
  };
  auto setSerials = [&](const long long* serial) {
    for (int k = 0; k < 3; ++k)
      if ((spec.matchMask >> k) & 1u) spec.matchSerial[k] = serial[k];
  };
  auto matchInLine = [&]() -> int {
    // all keypoint types are matched concurrently and nothing is read back: the number of matches arrives with the
    // optimizer's first evaluation.  A pending undistortion (of the working keypoints: the localization's) rides in this
    // iteration's search kernel (same keypoints, one launch less)
    if (undistortion.pending)
      LSA_TRY(lsa_match_types_undistorted(ctx, spec.target, spec.matchMask, &mp, pose.m, nullptr, undistortion.d0.m, undistortion.d1.m, Motion.Time0, Motion.Time1));
    else
      LSA_TRY(lsa_match_types(ctx, spec.target, spec.matchMask, spec.set, &mp, pose.m, nullptr));
    undistortion.pending = false;
    takeSerials(spec.matchSerial);
    return LSA_OK;
  };
  // iteration `iter` behind the link reserved last; 1 (and nothing enqueued) when it cannot wait there
  auto matchAhead = [&](unsigned iter, long long* serial) -> int {
    lsa_match_params_t next = mp;
    next.saturation_distance = saturation(iter);
    const int rc = lsa_match_types_linked(ctx, spec.target, spec.matchMask, spec.set, &next, spec.undistortAhead);
    if (rc == 0) takeSerials(serial);
    return rc;
  };

  for (; icpIter < spec.maxIter; ++icpIter)
  {
    Tick ticp;
    if (const int rc = top(icpIter); rc < 0) return rc;
    mp.saturation_distance = saturation(icpIter);
    LocalOptimizer optimizer(ctx);
    optimizer.SetDeviceLoop(DeviceLM);
    optimizer.SetTwoDMode(TwoDMode);
    optimizer.SetLMMaxIter(spec.lmMaxIter);
    optimizer.SetMinMatches(MinNbMatchedKeypoints);
    optimizer.UseDeviceResiduals(spec.solveMask);
    optimizer.SetPosePrior(pose);
    bool begun = false;  // the solve of this iteration is in flight
    if (icpIter < chained)
    {
      begun = true;
      setSerials(chainSerial[icpIter]);
    }
    else
    {
      if (const int rc = matchInLine(); rc < 0) return rc;
      if (chain)
      {
        // this iteration's solve and every iteration behind it, as far as they can ride behind links
        double prior[6];
        ToXYZRPY(pose, prior);
        lsa_icp_link_t link = spec.link;
        for (unsigned j = icpIter; j < spec.maxIter; ++j)
        {
          int leave = j + 1 < spec.maxIter ? lsa_icp_link(ctx) : -1;
          if (leave < 0) leave = -1;
          link.first = j == icpIter ? 1 : 0;
          const int rc = lsa_solve_device_begin_linked(ctx, spec.solveMask, j == icpIter ? prior : nullptr, TwoDMode ? 1 : 0, static_cast<int>(spec.lmMaxIter), static_cast<int>(MinNbMatchedKeypoints), leave,
                                                       leave >= 0 ? &link : nullptr);
          if (rc < 0) return Fail(rc, "lsa_solve_device_begin_linked");
          chained = j + 1;
          if (leave < 0) break;
          const int mrc = matchAhead(j + 1, chainSerial[j + 1]);
          if (mrc < 0) return Fail(mrc, "lsa_match_types_linked");
          if (mrc != 0) { lsa_icp_cancel(ctx, leave); break; }  // this match cannot wait behind a link: the loop goes on in line from there
        }
        chain = false;  // (enqueued once; whatever is not in the queue now runs in line)
        begun = true;
      }
    }
    ICP_TRACE("[%s %u] top: begun %d chained %u\n", spec.name, icpIter, (int)begun, chained);
    if (const int rc = enqueued(icpIter); rc < 0) return rc;
    if (!begun && own) ArmLookaheadInterlude();
    Stats.*spec.icpSeconds += ticp.Stop();
    (Stats.*spec.iterations)++;

    Tick tlm;
    SolveSummary summary;
    if (begun)
    {
      const int irc = InterludeWork();
      const int rc = optimizer.End(summary);
      ICP_TRACE("[%s %u] End rc %d irc %d\n", spec.name, icpIter, rc, irc);
      if (rc < 0) return Fail(rc, "LocalOptimizer::End");
      if (rc == 1) chained = 0;  // solved on the host: what was enqueued ahead has been called off
      if (irc < 0) return irc;
    }
    else
    {
      LSA_TRY(optimizer.Solve(summary));
      if (own) LSA_TRY(FinishLookaheadInterlude());
    }
    TotalMatchedKeypoints = summary.num_matches;
    if (lsa_icp_trace_on())
      std::fprintf(stderr, "[icp] frame %u %s %u: matches %d evals %d steps %d cost %.17g -> %.17g%s\n", NbrFrameProcessed, spec.name, icpIter, summary.num_matches, summary.num_evaluations,
                   summary.num_successful_steps, summary.initial_cost, summary.final_cost, summary.skipped ? " skipped" : "");
    if (const int rc = solved(); rc < 0) return rc;
    if (!summary.skipped || spec.countSkippedEvals) Stats.lm_evals += summary.num_evaluations;
    if (!summary.skipped) pose = optimizer.GetOptimizedPose();
    // Nothing more to search: called off HERE, in front of whatever `accepted` and `finished` put on the stream (an
    // undistortion, the registration error), so that what the links' matches announced on the host is taken back first.
    const bool last = summary.skipped || summary.num_successful_steps == 1 || icpIter + 1 == spec.maxIter;
    if (last) callOffRest(false);
    const int rc = summary.skipped ? skipped() : accepted(last, undistortion);
    Stats.*spec.lmSeconds += tlm.Stop();
    if (rc < 0) return rc;
    if (last)
    {
      if (const int frc = summary.skipped ? LSA_OK : finished(optimizer); frc < 0) return frc;
      break;
    }
    if (icpIter + 1 < chained)
      undistortion.pending = false;  // the next search is in the queue and undistorts with what the device worked out (the same)
  }
  atExit.failed = false;
  return LSA_OK;
}

}  // namespace host
}  // namespace lsa
