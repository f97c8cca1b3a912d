// lsa_slam_log.cpp -- the keypoint log of SlamCore and the calls that work on it: the trajectory put back with the maps
// rebuilt, place recognition, the two pose-graph optimizations, the registration of two logged frames.
#include "lsa_slam_icp_loop.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include "../lsa_device_grid_io.h"
#include "../lsa_kplog_io.h"
#include "lsa_pose_graph.h"

namespace lsa
{
namespace host
{
// Slam::LogCurrentFrameState (Slam.cxx:1225-1264).  The raw keypoints go into the device's log (lsa_kplog.hip): one
// launch on the registration stream, nothing of it with LoggingTimeout == 0
void SlamCore::LogCurrentFrameState(double time)
{
  LogTrajectory.push_back({Tworld, time});
  if (LoggingTimeout != 0.)
  {
    LogCovariances.push_back(LocalizationUncertainty.Covariance);
    if (!KpLogStopped && lsa_kplog_append(Ctx) < 0)
    {
      // the frame itself is done: the failure is reported, and the log says it no longer covers the trajectory
      KpLogStopped = true;
      LastError = std::string("keypoint logging stopped: ") + lsa_last_error(Ctx);
    }
    if (LoggingTimeout > 0)
      while (time - LogTrajectory.front().time > LoggingTimeout && LogTrajectory.size() > 2)
      {
        // (the log's frames are those of the newest poses: it drops its oldest only when it covers the oldest pose)
        if (!KpLogStopped && lsa_kplog_size(Ctx) == static_cast<int>(LogTrajectory.size())) (void)lsa_kplog_pop_front(Ctx);
        LogTrajectory.pop_front();
        LogCovariances.pop_front();
      }
  }
  else
    while (LogTrajectory.size() > 2) LogTrajectory.pop_front();
}

int SlamCore::LoggedFrames() const { return Ctx && !KpLogStopped ? lsa_kplog_size(Ctx) : 0; }

int SlamCore::GetLoggedKeypoints(int frame, int type, std::vector<lsa_point_t>& out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  out.clear();
  if (type < 0 || type > 2 || frame < 0 || frame >= LoggedFrames()) { LastError = "GetLoggedKeypoints: no such frame or keypoint type"; return LSA_E_ARG; }
  const int n = lsa_kplog_count(Ctx, frame, type);
  out.resize(std::max(n, 0));
  if (n > 0) LSA_TRY(lsa_kplog_get(Ctx, frame, type, out.data(), n));
  return n;
}

// ---- what the calls on the log share ------------------------------------------------------------------------------------------
int SlamCore::LogReady(const std::string& who, const char* whatIsMissing, bool covering)
{
  if (LoggingTimeout == 0.) { LastError = who + "keypoint logging is off (LoggingTimeout = 0): " + whatIsMissing; return LSA_E_STATE; }
  if (KpLogStopped) { LastError = who + "keypoint logging stopped when a chunk could not be allocated; Reset(true) starts it again"; return LSA_E_STATE; }
  if (covering)
    if (const int rc = LogCovers(who); rc < 0) return rc;
  return static_cast<int>(LogTrajectory.size());
}

int SlamCore::LogCovers(const std::string& who)
{
  if (lsa_kplog_size(Ctx) == static_cast<int>(LogTrajectory.size())) return LSA_OK;
  LastError = who + "the keypoint log does not cover the logged poses (logging was switched on after the first of them)";
  return LSA_E_STATE;
}

void SlamCore::LoggedPoses16(std::vector<double>& poses, std::vector<double>* times) const
{
  const size_t n = LogTrajectory.size();
  poses.resize(16 * n);
  if (times) times->resize(n);
  for (size_t i = 0; i < n; ++i)
  {
    std::memcpy(&poses[16 * i], LogTrajectory[i].pose.m, 16 * sizeof(double));
    if (times) (*times)[i] = LogTrajectory[i].time;
  }
}

std::vector<double> SlamCore::RowsOf(const double* poses16, int n) const
{
  std::vector<double> rows(static_cast<size_t>(n) * 17);
  for (int i = 0; i < n; ++i)
  {
    std::memcpy(&rows[17 * static_cast<size_t>(i)], poses16 + 16 * static_cast<size_t>(i), 16 * sizeof(double));
    rows[17 * static_cast<size_t>(i) + 16] = LogTrajectory[i].time;
  }
  return rows;
}

// Slam::RunPoseGraphOptimization from "Update SLAM trajectory and maps" on (Slam.cxx:404-477); the optimizer is the caller's
int SlamCore::SetTrajectoryAndRebuildMaps(const double* poses17, int n)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "SetTrajectoryAndRebuildMaps: ";
  const int logged = LogReady(who, "there is nothing to rebuild the maps from", false);
  if (logged < 0) return logged;
  if (!poses17 || n != logged) { LastError = who + std::to_string(n) + " poses for " + std::to_string(logged) + " logged ones"; return LSA_E_ARG; }
  if (n < 2) { LastError = who + "at least two poses"; return LSA_E_ARG; }
  for (int i = 0; i < n; ++i)
    if (!(poses17[17 * i + 16] == LogTrajectory[i].time))
    {
      LastError = who + "pose " + std::to_string(i) + " is not dated like the logged one";
      return LSA_E_ARG;
    }
  if (const int rc = LogCovers(who); rc < 0) return rc;
  // (one Add per type, of any size the replay addresses: a long log takes the form of the device maps' insertion that keeps its
  //  scans in global memory, lsa_grid_add.hip)
  std::vector<double> poses(static_cast<size_t>(n) * 16), times(n);
  for (int i = 0; i < n; ++i)
  {
    std::memcpy(&poses[16 * static_cast<size_t>(i)], poses17 + 17 * static_cast<size_t>(i), 16 * sizeof(double));
    times[i] = poses17[17 * static_cast<size_t>(i) + 16];
  }
  // "DenseMapOnTrajectory" 1: the dense map's corrections, against the logged poses while they still stand
  std::vector<double> denseCorrections;
  int denseFirstOrdinal = 0;
  const bool reproject = DenseCorrections(poses.data(), n, denseCorrections, &denseFirstOrdinal);
  // the map workers and the look-ahead are waited for, then what Reset(false) does (Slam.cxx:408)
  Reset(false, reproject);
  for (int i = 0; i < n; ++i) std::memcpy(LogTrajectory[i].pose.m, &poses[16 * static_cast<size_t>(i)], 16 * sizeof(double));
  // (before the replay: whatever fails behind it, the dense map stands under the poses the log now holds, or is empty)
  const int denseRc = reproject ? ReprojectDenseMap(denseCorrections, denseFirstOrdinal) : LSA_OK;
  const std::string denseError = LastError;
  const unsigned mask = UsedTypesMask();
  float mn[3][3], mx[3][3];
  const int undistort = Undistortion != UNDISTORTION_NONE ? 1 : 0;
  if (DeviceMapsInUse())
  {
    lsa_device_grid* grids[3];
    for (int k = 0; k < 3; ++k) grids[k] = UseKeypoints[k] ? DevMaps[k] : nullptr;
    LSA_TRY(lsa_kplog_replay_to_grids(Ctx, mask, poses.data(), times.data(), n, undistort, grids, mn, mx));
    for (int k = 0; k < 3; ++k)
      if (UseKeypoints[k]) LSA_TRY(lsa_device_grid_roll(DevMaps[k], mn[k], mx[k]));
  }
  else
  {
    LSA_TRY(lsa_kplog_replay(Ctx, mask, poses.data(), times.data(), n, undistort, nullptr, mn, mx));
    for (int k = 0; k < 3; ++k)
    {
      if (!UseKeypoints[k]) continue;
      const lsa_point_t* pts = nullptr;
      const long long cnt = lsa_kplog_replayed(Ctx, k, &pts);
      if (cnt > 0) LocalMaps[k]->Add(pts, static_cast<std::size_t>(cnt), false, -1., false);
      LocalMaps[k]->Roll(mn[k], mx[k]);
    }
  }
  std::memcpy(Tworld.m, &poses[16 * static_cast<size_t>(n - 1)], 16 * sizeof(double));
  std::memcpy(PreviousTworld.m, &poses[16 * static_cast<size_t>(n - 2)], 16 * sizeof(double));
  // the trajectory is applied; a re-projection that failed for another reason than memory is the call's answer (map cleared)
  if (denseRc < 0) LastError = denseError;
  return denseRc;
}

// ---- place recognition: which logged frame looks like this one (descriptors of the keypoint log, lsa_place.hip) -------------
int SlamCore::RecognizePlace(int query, const lsa_place_search_t* search, lsa_place_candidate_t* out, int capacity)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "RecognizePlace: ";
  if (capacity < 0 || (capacity > 0 && !out)) { LastError = who + "no place for the candidates"; return LSA_E_ARG; }
  const int n = LogReady(who, "there are no logged keypoints to describe");
  if (n < 0) return n;
  lsa_place_search_t p;
  lsa_place_search_init(&p);
  if (search) p = *search;
  if (query < 0 || query >= n) { LastError = who + "query frame " + std::to_string(query) + " is not one of the " + std::to_string(n) + " logged ones"; return LSA_E_ARG; }
  if (!place::params_ok(p.descriptor) || !(p.min_travelled >= 0.) || p.exclusion_half_window < 0 || p.max_distance != p.max_distance ||
      p.max_descriptor_distance != p.max_descriptor_distance)
  {
    LastError = who + "parameters out of limits";
    return LSA_E_ARG;
  }
  if (query == 0) return 0;  // no frame before it
  // the device works from here on: the map workers and the look-ahead have enqueued what they had (nothing of theirs is changed)
  WaitMaps();
  std::vector<float> distance(static_cast<size_t>(query));
  std::vector<int32_t> shift(static_cast<size_t>(query));
  if (const int rc = lsa_kplog_place_search(Ctx, &p.descriptor, query, 0, query - 1, distance.data(), shift.data()); rc < 0)
  {
    LastError = who + lsa_last_error(Ctx);
    return rc;
  }
  std::vector<double> poses;
  LoggedPoses16(poses, nullptr);
  const std::vector<double> rows = RowsOf(poses.data(), n);
  const int found = PlaceSelect(distance.data(), shift.data(), rows.data(), n, query, p.descriptor.sectors, p.min_travelled, p.max_distance, p.max_descriptor_distance,
                                p.exclusion_half_window, out, capacity);
  if (found < 0) LastError = who + "bad argument";
  return found;
}

// ---- loop detection over the whole log: RecognizePlace for a set of queries in one pass (lsa_place_detect.hip) --------------
int SlamCore::DetectLoopClosures(const lsa_loop_detect_t* detect, lsa_loop_candidate_t* out, int capacity)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "DetectLoopClosures: ";
  if (capacity < 0 || (capacity > 0 && !out)) { LastError = who + "no place for the candidates"; return LSA_E_ARG; }
  const int n = LogReady(who, "there are no logged keypoints to describe");
  if (n < 0) return n;
  lsa_loop_detect_t d;
  lsa_loop_detect_init(&d);
  if (detect) d = *detect;
  int last = 0;
  if (DetectQueries(d, n, capacity, &last) < 0)
  {
    LastError = who + "a query set outside the " + std::to_string(n) + " logged frames, per_query outside 1..16, room for fewer than queries * per_query candidates, or parameters out of limits";
    return LSA_E_ARG;
  }
  // the device works from here on: the map workers and the look-ahead have enqueued what they had (nothing of theirs is changed)
  WaitMaps();
  std::vector<double> poses;
  LoggedPoses16(poses, nullptr);
  const std::vector<double> rows = RowsOf(poses.data(), n);
  const int found = lsa_kplog_detect_loops(Ctx, &d, rows.data(), n, out, capacity);
  if (found < 0) LastError = who + lsa_last_error(Ctx);
  return found;
}

// ---- detect, register, solve, apply: the calls above and below, composed (lsa_slam_close_loops) ------------------------------
int SlamCore::CloseLoops(const lsa_loop_detect_t* detect, const lsa_loop_closure_params_t* loopParams, const lsa_pgo_params_t* pgoParams, const lsa_pgo_robust_t* robust,
                         double* poses17, int capacity, lsa_pgo_result_t* result, lsa_loop_report_t* reports, int reportCapacity)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "CloseLoops: ";
  if (!poses17 || !result || reportCapacity < 0 || (reportCapacity > 0 && !reports)) { LastError = who + "bad argument"; return LSA_E_ARG; }
  // what the solve would refuse is refused before anything runs: a refusal changes nothing
  const int n = LogReady(who, "there is no logged trajectory to optimize");
  if (n < 0) return n;
  lsa_pgo_params_t pp;
  lsa_pgo_params_init(&pp);
  if (pgoParams) pp = *pgoParams;
  if (!pg::params_ok(pp) || (robust && !pg::robust_ok(*robust))) { LastError = who + "pose-graph parameters out of limits, a loss outside 0..3, or a scale that is not finite and positive"; return LSA_E_ARG; }
  if (n < 2) { LastError = who + "at least two logged poses"; return LSA_E_ARG; }
  if (capacity < n) { LastError = who + "room for " + std::to_string(capacity) + " of " + std::to_string(n) + " poses"; return LSA_E_ARG; }
  std::vector<lsa_loop_candidate_t> found(static_cast<size_t>(reportCapacity));
  const int m = DetectLoopClosures(detect, found.data(), reportCapacity);
  if (m < 0) return m;
  std::vector<lsa_loop_report_t> rep(static_cast<size_t>(m));
  std::vector<lsa_pgo_edge_t> edges;
  for (int k = 0; k < m; ++k)
  {
    const lsa_loop_candidate_t& c = found[static_cast<size_t>(k)];
    lsa_loop_report_t& r = rep[static_cast<size_t>(k)];
    std::memset(&r, 0, sizeof(r));
    r.query = c.query;
    r.frame = c.frame;
    r.distance = c.distance;
    r.yaw = c.yaw;
    r.edge = -1;
    r.weight = -1.;
    // the start: the revisited frame's pose with the base turned by the descriptors' yaw, P[frame] * Rz(yaw)
    Pose rz = Pose::Identity();
    rz(0, 0) = std::cos(c.yaw);
    rz(0, 1) = -std::sin(c.yaw);
    rz(1, 0) = std::sin(c.yaw);
    rz(1, 1) = std::cos(c.yaw);
    const Pose guess = LogTrajectory[c.frame].pose * rz;
    lsa_loop_closure_result_t reg;
    const int rc = RegisterLoggedFrames(c.query, c.frame, loopParams, guess.m, &reg);
    r.status = rc < 0 ? rc : reg.status;
    if (rc < 0) continue;  // (windows that overlap, say: the candidate is reported, no edge comes of it)
    r.iterations = reg.iterations;
    r.position_error = reg.position_error;
    lsa_pgo_edge_t ed;
    std::memset(&ed, 0, sizeof(ed));
    ed.from = c.frame;
    ed.to = c.query;
    std::memcpy(ed.relative, reg.relative, sizeof(ed.relative));
    if (reg.status != 0 || lsa_pgo_information_from_covariance(reg.covariance, ed.information) != LSA_OK) continue;
    r.edge = static_cast<int>(edges.size());
    edges.push_back(ed);
  }
  if (edges.empty())
  {
    // nothing to solve: the poses as they are logged, a summary that says so
    std::vector<double> poses;
    LoggedPoses16(poses, nullptr);
    const std::vector<double> rows = RowsOf(poses.data(), n);
    std::memcpy(poses17, rows.data(), rows.size() * sizeof(double));
    std::memset(result, 0, sizeof(*result));
    result->message = m == 0 ? "no loop candidate: nothing to solve" : "no loop edge: nothing to solve";
  }
  else
  {
    std::vector<double> verdict(2 * edges.size());
    const int rc = OptimizeLoggedTrajectory(edges.data(), static_cast<int>(edges.size()), &pp, poses17, capacity, result, robust, verdict.data());
    if (rc < 0) return rc;
    for (lsa_loop_report_t& r : rep)
      if (r.edge >= 0)
      {
        r.chi2 = verdict[2 * static_cast<size_t>(r.edge)];
        r.weight = verdict[2 * static_cast<size_t>(r.edge) + 1];
      }
  }
  LastError.clear();  // (a refused registration left its reason; the call as a whole went through, and its reports say the rest)
  if (m > 0) std::memcpy(reports, rep.data(), static_cast<size_t>(m) * sizeof(lsa_loop_report_t));
  return m;
}

// ---- pose-graph optimization of the logged trajectory (lsa_pose_graph.hip) ---------------------------------------------------
// the odometry chain of the log: edge i-1 -> i with Z = inv(P[i-1]) P[i], weighted by p.odometry_information (n - 1 edges)
int SlamCore::LoggedChainEdges(const lsa_pgo_params_t& p, const std::string& who, lsa_pgo_edge_t* edges)
{
  const int n = static_cast<int>(LogTrajectory.size());
  double diagonal[36];
  std::memset(diagonal, 0, sizeof(diagonal));
  if (p.odometry_information == 0)
    for (int k = 0; k < 6; ++k)
    {
      const double sigma = p.odometry_sigma[k];
      if (!(sigma > 0.) || !pg::finite_d(1. / (sigma * sigma))) { LastError = who + "odometry_sigma must be positive"; return LSA_E_ARG; }
      diagonal[k * 7] = 1. / (sigma * sigma);
    }
  else if (static_cast<int>(LogCovariances.size()) != n) { LastError = who + "the covariance log does not cover the logged poses (odometry_information 0 needs none)"; return LSA_E_STATE; }
  for (int i = 1; i < n; ++i)
  {
    lsa_pgo_edge_t& ed = edges[static_cast<size_t>(i - 1)];
    ed.from = i - 1;
    ed.to = i;
    const Pose z = Inverse(LogTrajectory[i - 1].pose) * LogTrajectory[i].pose;
    std::memcpy(ed.relative, z.m, sizeof(ed.relative));
    if (p.odometry_information == 0) std::memcpy(ed.information, diagonal, sizeof(diagonal));
    else if (lsa_pgo_information_from_covariance(LogCovariances[i].data(), ed.information) != LSA_OK)
    {
      LastError = who + "the logged covariance of frame " + std::to_string(i) + " is not positive definite (odometry_information 0 needs none)";
      return LSA_E_ARG;
    }
  }
  return LSA_OK;
}

// What OptimizeLoggedTrajectory and RunPoseGraphOptimization hand their solve: the checked parameters, the logged poses
// (16 doubles each) with their times, the chain edges with the call's own loop edges behind them
struct SlamCore::PoseGraphProblem
{
  lsa_pgo_params_t p;
  std::vector<double> in, times;
  std::vector<lsa_pgo_edge_t> edges;
};

// Both calls, after their own argument checks: the log's refusals, the parameters (the defaults without `params`) within
// their limits, `tooFew` (the call's own words for a track of fewer than two points; empty: there are enough), room for the
// poses.  Returns the number of logged poses, packed into pb.
int SlamCore::PoseGraphBegin(const std::string& who, const lsa_pgo_params_t* params, const std::string& tooFew, int capacity, PoseGraphProblem& pb)
{
  const int n = LogReady(who, "there is no logged trajectory to optimize");
  if (n < 0) return n;
  lsa_pgo_params_init(&pb.p);
  if (params) pb.p = *params;
  if (!pg::params_ok(pb.p)) { LastError = who + "parameters out of limits"; return LSA_E_ARG; }
  if (!tooFew.empty()) { LastError = who + tooFew; return LSA_E_ARG; }
  if (capacity < n) { LastError = who + "room for " + std::to_string(capacity) + " of " + std::to_string(n) + " poses"; return LSA_E_ARG; }
  LoggedPoses16(pb.in, &pb.times);
  return n;
}

// ... and once their own inputs are in order: the graph's edges, held to the poses they join
int SlamCore::PoseGraphEdges(const std::string& who, const lsa_pgo_edge_t* loopEdges, int m, PoseGraphProblem& pb)
{
  const int n = static_cast<int>(pb.times.size());
  pb.edges.resize(static_cast<size_t>(n - 1 + m));
  if (const int rc = LoggedChainEdges(pb.p, who, pb.edges.data()); rc != LSA_OK) return rc;
  for (int k = 0; k < m; ++k) pb.edges[static_cast<size_t>(n - 1 + k)] = loopEdges[k];
  std::string why;
  if (const int rc = PgoCheckEdges(pb.in.data(), n, pb.edges.data(), static_cast<int>(pb.edges.size()), &why); rc != LSA_OK) { LastError = who + why; return rc; }
  return LSA_OK;
}

// From the solve on.  solve(out16, result) runs on LoopCtx and returns an LSA_* code; with p.apply its poses go through
// SetTrajectoryAndRebuildMaps.  Returns the number of poses written to poses17.
template <class Solve>
int SlamCore::PoseGraphSolve(const std::string& who, const PoseGraphProblem& pb, const Solve& solve, double* poses17, lsa_pgo_result_t* result)
{
  const int n = static_cast<int>(pb.times.size());
  std::vector<double> out(pb.in.size());
  // from here on the device works: the map workers and the look-ahead have enqueued what they had (nothing of theirs is changed)
  WaitMaps();
  if (const int rc = EnsureLoopClosureScratch(); rc < 0) return rc;
  (void)lsa_collect_garbage(LoopCtx);
  Tick t;
  lsa_pgo_result_t r;
  if (const int rc = solve(out.data(), &r); rc < 0)
  {
    LastError = who + lsa_last_error(LoopCtx);
    return rc;
  }
  PoseGraphSeconds = t.Stop();
  const std::vector<double> rows = RowsOf(out.data(), n);
  if (pb.p.apply != 0)
    if (const int rc = SetTrajectoryAndRebuildMaps(rows.data(), n); rc < 0) return rc;
  std::memcpy(poses17, rows.data(), rows.size() * sizeof(double));
  *result = r;
  return n;
}

int SlamCore::OptimizeLoggedTrajectory(const lsa_pgo_edge_t* loopEdges, int m,const lsa_pgo_params_t* params, double* poses17, int capacity, lsa_pgo_result_t* result,
                                       const lsa_pgo_robust_t* robust, double* loopVerdict)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "OptimizeLoggedTrajectory: ";
  if (!result || !poses17 || m < 0 || (m > 0 && !loopEdges)) { LastError = who + "bad argument"; return LSA_E_ARG; }
  PoseGraphProblem pb;
  const int n = PoseGraphBegin(who, params, LogTrajectory.size() < 2 ? "at least two logged poses" : "", capacity, pb);
  if (n < 0) return n;
  if (robust && !pg::robust_ok(*robust)) { LastError = who + "a loss outside 0..3, or a scale that is not finite and positive"; return LSA_E_ARG; }
  for (int k = 0; k < m; ++k)
    if (loopEdges[k].from < 0 || loopEdges[k].from >= n || loopEdges[k].to < 0 || loopEdges[k].to >= n || loopEdges[k].from == loopEdges[k].to)
    {
      LastError = who + "loop edge " + std::to_string(k) + " does not join two of the " + std::to_string(n) + " logged poses";
      return LSA_E_ARG;
    }
  if (const int rc = PoseGraphEdges(who, loopEdges, m, pb); rc != LSA_OK) return rc;
  std::vector<unsigned char> fixed(static_cast<size_t>(n), 0);
  fixed[0] = 1;
  // the losses act on the caller's loop edges alone: the odometry chain keeps the graph connected and is never discounted
  std::vector<unsigned char> mask(pb.edges.size(), 0);
  for (int k = 0; k < m; ++k) mask[static_cast<size_t>(n - 1 + k)] = 1;
  std::vector<double> verdict(loopVerdict ? 2 * pb.edges.size() : 0);
  auto solve = [&](double* out, lsa_pgo_result_t* r) {
    return lsa_pgo_solve_robust(LoopCtx, pb.in.data(), n, fixed.data(), pb.edges.data(), static_cast<int>(pb.edges.size()), mask.data(), nullptr, 0, nullptr, &pb.p, robust, out, r,
                                loopVerdict ? verdict.data() : nullptr, nullptr);
  };
  const int rc = PoseGraphSolve(who, pb, solve, poses17, result);
  if (rc >= 0 && loopVerdict && m > 0) std::memcpy(loopVerdict, verdict.data() + 2 * static_cast<size_t>(n - 1), 2 * static_cast<size_t>(m) * sizeof(double));
  return rc;
}

// ---- Slam::RunPoseGraphOptimization (Slam.cxx:355-477, PoseGraphOptimization::Process): GPS positions as priors -------------
int SlamCore::RunPoseGraphOptimization(const double* gpsTimes, const double* gpsXyz, const double* gpsCov9, int G, double* gpsToSensor16, double timeOffset,
                                       const lsa_pgo_params_t* params, double* poses17, int capacity, lsa_pgo_result_t* result, const lsa_pgo_robust_t* robust,
                                       double* fixVerdict)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "RunPoseGraphOptimization: ";
  if (!result || !poses17 || !gpsToSensor16 || G < 0 || (G > 0 && (!gpsTimes || !gpsXyz || !gpsCov9)) || !pg::finite_d(timeOffset)) { LastError = who + "bad argument"; return LSA_E_ARG; }
  std::string tooFew;
  if (LogTrajectory.size() < 2 || G < 2)
    tooFew = "the SLAM and GPS trajectories must have at least 2 points (got " + std::to_string(LogTrajectory.size()) + " logged poses and " + std::to_string(G) + " GPS positions)";
  PoseGraphProblem pb;
  const int n = PoseGraphBegin(who, params, tooFew, capacity, pb);
  if (n < 0) return n;
  if (robust && !pg::robust_ok(*robust)) { LastError = who + "a loss outside 0..3, or a scale that is not finite and positive"; return LSA_E_ARG; }
  const std::vector<double>& times = pb.times;
  for (int k = 0; k < 16; ++k)
    if (!pg::finite_d(gpsToSensor16[k])) { LastError = who + "the GPS to sensor calibration has a non-finite entry"; return LSA_E_ARG; }
  for (int f = 0; f < G; ++f)
    for (int k = 0; k < 3; ++k)
      if (!pg::finite_d(gpsXyz[3 * static_cast<size_t>(f) + k]) || !pg::finite_d(gpsTimes[f])) { LastError = who + "GPS fix " + std::to_string(f) + " has a non-finite entry"; return LSA_E_ARG; }
  // the two tracks must overlap in time (PoseGraphOptimization.cxx:130-143; the logged times carry the offset here, and the
  // intervals are closed: the reference's strict comparison refuses two tracks that begin at the same instant, an accident)
  {
    const double g0 = gpsTimes[0], g1 = gpsTimes[G - 1], s0 = times[0] + timeOffset, s1 = times[static_cast<size_t>(n) - 1] + timeOffset;
    auto inside = [](double t, double lo, double hi) { return lo <= t && t <= hi; };
    if (!inside(g0, s0, s1) && !inside(s0, g0, g1))
    {
      LastError = who + "SLAM time and GPS time do not match: GPS = (" + std::to_string(g0) + ", " + std::to_string(g1) + "), SLAM = (" + std::to_string(s0) + ", " +
                  std::to_string(s1) + "); please indicate the time offset";
      return LSA_E_ARG;
    }
  }
  std::vector<int32_t> match(static_cast<size_t>(G));
  if (lsa_gps_match_trajectory(times.data(), n, gpsTimes, G, timeOffset, 0.1, match.data()) != LSA_OK) { LastError = who + "the logged or the GPS times are not ascending"; return LSA_E_ARG; }
  // O = inverse(gpsToSensor) is what the reference hands g2o's ParameterSE3Offset (PoseGraphOptimization.cxx:102-106): the fix of
  // pose P is expected at the translation of P O
  Pose cal;
  std::memcpy(cal.m, gpsToSensor16, sizeof(cal.m));
  const Pose offset = Inverse(cal);
  std::vector<lsa_pgo_prior_t> priors;
  std::vector<double> from, to;
  for (int f = 0; f < G; ++f)
  {
    if (match[static_cast<size_t>(f)] < 0) continue;
    lsa_pgo_prior_t pr;
    std::memset(&pr, 0, sizeof(pr));
    pr.pose = match[static_cast<size_t>(f)];
    std::memcpy(pr.position, gpsXyz + 3 * static_cast<size_t>(f), sizeof(pr.position));
    if (lsa_pgo_information_from_covariance3(gpsCov9 + 9 * static_cast<size_t>(f), pr.information) != LSA_OK)
    {
      LastError = who + "the covariance of GPS fix " + std::to_string(f) + " is not positive definite";
      return LSA_E_ARG;
    }
    priors.push_back(pr);
    const Pose antenna = LogTrajectory[pr.pose].pose * offset;  // its translation: t_i + R_i t_o
    for (int k = 0; k < 3; ++k) { from.push_back(antenna.m[4 * k + 3]); to.push_back(pr.position[k]); }
  }
  if (priors.empty()) { LastError = who + "no GPS fix is within 0.1 s of a logged pose"; return LSA_E_ARG; }
  double W[16];
  if (lsa_trajectory_alignment(from.data(), to.data(), static_cast<int>(priors.size()), W) != LSA_OK) { LastError = who + "the two tracks could not be aligned"; return LSA_E_ARG; }
  if (const int rc = PoseGraphEdges(who, nullptr, 0, pb); rc != LSA_OK) return rc;
  std::vector<double> start(pb.in.size()), opt(pb.in.size());
  std::vector<unsigned char> fixed(static_cast<size_t>(n), 0);  // every pose is free: the priors hold the graph
  // prior_loss acts on the GPS priors; the odometry chain is never discounted
  lsa_pgo_robust_t rb;
  lsa_pgo_robust_init(&rb);
  if (robust) { rb.prior_loss = robust->prior_loss; rb.prior_scale = robust->prior_scale; }
  std::vector<double> verdict(fixVerdict ? 2 * priors.size() : 0);
  auto solve = [&](double* out, lsa_pgo_result_t* r) {
    int rc = lsa_pgo_premultiply(LoopCtx, pb.in.data(), n, W, start.data());
    if (rc == LSA_OK)
      rc = lsa_pgo_solve_robust(LoopCtx, start.data(), n, fixed.data(), pb.edges.data(), n - 1, nullptr, priors.data(), static_cast<int>(priors.size()), offset.m, &pb.p, &rb, opt.data(), r,
                                nullptr, fixVerdict ? verdict.data() : nullptr);
    if (rc == LSA_OK) rc = lsa_pgo_reanchor(LoopCtx, opt.data(), n, out);
    return rc;
  };
  const int rc = PoseGraphSolve(who, pb, solve, poses17, result);
  if (rc < 0) return rc;
  std::memcpy(gpsToSensor16, opt.data(), 16 * sizeof(double));  // the optimized pose 0 in the GPS frame (Slam.cxx:404)
  if (fixVerdict)
    for (int f = 0, a = 0; f < G; ++f)
    {
      const bool matched = match[static_cast<size_t>(f)] >= 0;
      fixVerdict[2 * static_cast<size_t>(f)] = matched ? verdict[2 * static_cast<size_t>(a)] : 0.;
      fixVerdict[2 * static_cast<size_t>(f) + 1] = matched ? verdict[2 * static_cast<size_t>(a) + 1] : -1.;
      a += matched ? 1 : 0;
    }
  return rc;
}

// ---- loop closure: a logged frame registered against the log around a revisited pose ---------------------------------------
int SlamCore::EnsureLoopClosureScratch()
{
  if (LoopCtx) return LSA_OK;
  lsa_ctx* ctx = nullptr;
  const int rc = lsa_ctx_create(Ctx->device, &ctx);
  if (rc != LSA_OK) { LastError = "RegisterLoggedFrames: the scratch context could not be created"; return rc; }
  for (int k = 0; k < 3; ++k)
    if (const int grc = lsa_device_grid_create(ctx, &LoopMaps[k]); grc != LSA_OK)
    {
      LastError = std::string("RegisterLoggedFrames: a scratch map could not be created: ") + lsa_last_error(ctx);
      for (auto*& g : LoopMaps) { if (g) lsa_device_grid_destroy(g); g = nullptr; }
      lsa_ctx_destroy(ctx);
      return grc;
    }
  LoopCtx = ctx;
  return LSA_OK;
}

int SlamCore::RegisterLoggedFrames(int query, int revisited, const lsa_loop_closure_params_t* params, const double* guess16, lsa_loop_closure_result_t* out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "RegisterLoggedFrames: ";
  if (!out) { LastError = who + "no place for the result"; return LSA_E_ARG; }
  const int n = LogReady(who, "there are no logged keypoints to register against");
  if (n < 0) return n;
  lsa_loop_closure_params_t p;
  std::memset(&p, 0, sizeof(p));
  p.revisited_half_window = 5;
  if (params) p = *params;
  LoopClosureWindows w;
  {
    std::string why;
    if (const int rc = LoopClosureWindowsOf(n, query, revisited, p.revisited_half_window, p.query_half_window, &w, &why); rc != LSA_OK) { LastError = who + why; return rc; }
  }
  if (!DevMaps[0] || !DevMaps[1] || !DevMaps[2]) { LastError = who + "no device maps to take the scratch maps' parameters from"; return LSA_E_STATE; }
  // from here on the device works: the map workers and the look-ahead have enqueued what they had (nothing of theirs is changed)
  Tick tall;
  double seconds[3] = {0., 0., 0.};  // replays, scratch maps, ICP
  WaitMaps();
  if (const int rc = EnsureLoopClosureScratch(); rc < 0) return rc;
  (void)lsa_collect_garbage(LoopCtx);  // what the last call outgrew (nothing on the device waits for the host here)
  auto failOn = [&](lsa_ctx* ctx, int rc, const char* where) {
    LastError = who + where + ": " + lsa_last_error(ctx);
    return rc;
  };

  const unsigned mask = UsedTypesMask();
  const int rule = Undistortion != UNDISTORTION_NONE ? 2 : 0;
  std::vector<double> poses, times;
  LoggedPoses16(poses, &times);
  std::memset(out, 0, sizeof(*out));
  float mn[3][3], mx[3][3];
  long long counts[3] = {0, 0, 0};

  // the target: the revisited frames under the logged trajectory, ONE Add(fixed = false, time = -1, roll = true) per type
  // into a fresh grid with that type's map parameters; the whole grid, unfiltered, is the sub-map
  for (int k = 0; k < 3; ++k)
    if (const int rc = grid_adopt_parameters(LoopMaps[k], DevMaps[k]); rc < 0) return failOn(LoopCtx, rc, "the scratch maps' parameters");
  {
    // (the replay waits for the log's stream; the insertions behind it are only enqueued: the sub-maps' sizes wait for them)
    const KpLogRange range{mask, poses.data(), times.data(), n, w.r0, w.r1, rule};
    Tick t;
    if (const int rc = kplog_replay_range_to_grids(Ctx, range, LoopMaps, false, -1., true, counts, mn, mx); rc < 0) return failOn(Ctx, rc, "the replay of the revisited frames");
    seconds[0] += t.Stop();
  }
  Tick tmaps;
  for (int k = 0; k < 3; ++k)
  {
    if (!UseKeypoints[k]) continue;
    lsa_set_target_cell_size(LoopCtx, LSA_TARGET_MAP, k, MapSearchCell(k));
    if (const int rc = lsa_device_grid_build_submap_begin(LoopMaps[k], nullptr, nullptr, -1, LSA_TARGET_MAP, k); rc < 0) return failOn(LoopCtx, rc, "lsa_device_grid_build_submap_begin");
  }
  for (int k = 0; k < 3; ++k)
  {
    if (!UseKeypoints[k]) continue;
    const int size = lsa_device_grid_build_submap_end(LoopMaps[k]);
    if (size < 0) return failOn(LoopCtx, size, "lsa_device_grid_build_submap_end");
    out->target_points[k] = size;
  }
  seconds[1] += tmaps.Stop();

  // the query: its frames under inv(P[q]) * P[i] -- q's BASE frame -- into the scratch context's working keypoints
  const Pose logged = LogTrajectory[query].pose;
  {
    const Pose inv = Inverse(logged);
    std::vector<double> rel(static_cast<size_t>(n) * 16, 0.);
    for (int i = std::max(w.q0 - 1, 0); i <= w.q1; ++i)
    {
      const Pose r = inv * LogTrajectory[i].pose;
      std::memcpy(&rel[16 * static_cast<size_t>(i)], r.m, 16 * sizeof(double));
    }
    const KpLogRange range{mask, rel.data(), times.data(), n, w.q0, w.q1, rule};
    Tick t;
    if (const int rc = kplog_replay_range_to_set(Ctx, range, LoopCtx, LSA_SET_WORKING, counts, mn, mx); rc < 0) return failOn(Ctx, rc, "the replay of the query frames");
    seconds[0] += t.Stop();
    for (int k = 0; k < 3; ++k) out->query_points[k] = counts[k];
  }
  Tick ticp;

  // the ICP loop of Localization() on the scratch context, strictly in line: no sensor terms, no undistortion in between
  Pose world = logged;
  if (guess16) std::memcpy(world.m, guess16, 16 * sizeof(double));
  // the search's form and tuning as the frame path has them (results do not depend on either)
  ApplySearchTuning(LoopCtx);
  long long serial[3] = {0, 0, 0};
  IcpLoopSpec spec = {};
  spec.name = "reg";
  spec.ctx = LoopCtx;
  spec.inLine = true;
  spec.target = LSA_TARGET_MAP;
  spec.set = LSA_SET_WORKING;
  spec.matchMask = spec.solveMask = mask;
  spec.maxIter = p.icp_max_iter > 0 ? static_cast<unsigned>(p.icp_max_iter) : LocalizationICPMaxIter;
  spec.lmMaxIter = p.lm_max_iter > 0 ? static_cast<unsigned>(p.lm_max_iter) : LocalizationLMMaxIter;
  spec.initSaturation = p.init_saturation > 0. ? p.init_saturation : LocalizationInitSaturationDistance;
  spec.finalSaturation = p.final_saturation > 0. ? p.final_saturation : LocalizationFinalSaturationDistance;
  spec.match = LocMatchParams();
  spec.matchSerial = serial;
  spec.icpSeconds = &FrameStats::loc_icp;
  spec.lmSeconds = &FrameStats::loc_lm;
  spec.iterations = &FrameStats::loc_iters;
  int iterations = 0;
  RegistrationError uncertainty;
  auto solved = [&]() -> int {
    // the rejection histograms of this iteration's matches (the first iteration's are kept, the last one's stay)
    for (int k = 0; k < 3; ++k)
    {
      if (!((mask >> k) & 1u)) continue;
      int h[LSA_MATCH_NSTATUS];
      if (const int rc = lsa_match_histogram(LoopCtx, k, serial[k], h); rc < 0) return failOn(LoopCtx, rc, "lsa_match_histogram");
      for (int s = 0; s < LSA_MATCH_NSTATUS; ++s)
      {
        if (iterations == 0) out->first_histogram[k][s] = h[s];
        out->last_histogram[k][s] = h[s];
      }
    }
    ++iterations;
    return LSA_OK;
  };
  auto skipped = [&]() -> int { out->status = 1; return LSA_OK; };
  auto finished = [&](LocalOptimizer& optimizer) -> int { return optimizer.EstimateRegistrationError(uncertainty); };
  // (the loop's counters are the frame path's: they are put back, the frame's statistics do not notice either)
  const FrameStats stats = Stats;
  const unsigned matched = TotalMatchedKeypoints;
  const std::string error = LastError;
  const int rc = RunIcpLoop(spec, world, kNothing, kNothing, solved, skipped, kNothing, finished);
  Stats = stats;
  TotalMatchedKeypoints = matched;
  if (rc < 0) return LastError.rfind(who, 0) == 0 ? rc : failOn(LoopCtx, rc, "the ICP loop");
  LastError = error;
  if (const int src = lsa_sync(LoopCtx); src < 0) return failOn(LoopCtx, src, "lsa_sync");
  seconds[2] = ticp.Stop();
  for (int i = 0; i < 3; ++i) LoopClosureSeconds[i] = seconds[i];
  LoopClosureSeconds[3] = tall.Stop();

  std::memcpy(out->world, world.m, sizeof(out->world));
  const Pose relative = Inverse(LogTrajectory[revisited].pose) * world;
  std::memcpy(out->relative, relative.m, sizeof(out->relative));
  std::memcpy(out->covariance, uncertainty.Covariance.data(), sizeof(out->covariance));
  out->position_error = uncertainty.PositionError;
  out->orientation_error = uncertainty.OrientationError;
  out->iterations = iterations;
  return LSA_OK;
}

}  // namespace host
}  // namespace lsa
