// lsa_slam_icp.cpp -- SlamCore's two registrations, ComputeEgoMotion() and Localization(), and the undistortion between
// their iterations.  The loop itself is lsa_slam_icp_loop.h.
#include "lsa_slam_icp_loop.h"
#include <cmath>
#include <cstring>

namespace lsa
{
namespace host
{
lsa_match_params_t SlamCore::EgoMatchParams() const
{
  lsa_match_params_t p;
  std::memset(&p, 0, sizeof(p));
  p.single_edge_per_ring = 1;  // Slam.cxx:879
  p.max_neighbors_distance = EgoMotionMaxNeighborsDistance;
  p.edge_nb_neighbors = EgoMotionEdgeNbNeighbors;
  p.edge_min_nb_neighbors = EgoMotionEdgeMinNbNeighbors;
  p.edge_max_model_error = EgoMotionEdgeMaxModelError;
  p.plane_nb_neighbors = EgoMotionPlaneNbNeighbors;
  p.planarity_threshold = EgoMotionPlanarityThreshold;
  p.plane_max_model_error = EgoMotionPlaneMaxModelError;
  p.blob_nb_neighbors = 10;
  p.saturation_distance = 1.;
  return p;
}
lsa_match_params_t SlamCore::LocMatchParams() const
{
  lsa_match_params_t p;
  std::memset(&p, 0, sizeof(p));
  p.single_edge_per_ring = 0;  // Slam.cxx:1057
  p.max_neighbors_distance = LocalizationMaxNeighborsDistance;
  p.edge_nb_neighbors = LocalizationEdgeNbNeighbors;
  p.edge_min_nb_neighbors = LocalizationEdgeMinNbNeighbors;
  p.edge_max_model_error = LocalizationEdgeMaxModelError;
  p.plane_nb_neighbors = LocalizationPlaneNbNeighbors;
  p.planarity_threshold = LocalizationPlanarityThreshold;
  p.plane_max_model_error = LocalizationPlaneMaxModelError;
  p.blob_nb_neighbors = LocalizationBlobNbNeighbors;
  p.saturation_distance = 1.;
  return p;
}

// MatchingResults::Rejections / Weights of the loop's last iteration (KeepMatchDebug)
int SlamCore::DownloadMatchDebug(int set, unsigned typeMask, MatchDebug* debug)
{
  for (int k = 0; k < 3; ++k)
  {
    if (!((typeMask >> k) & 1u)) continue;
    const int n = lsa_keypoint_count(Ctx, set, k);
    debug[k].status.assign(n, LSA_MATCH_UNKOWN);
    debug[k].weights.assign(n, 0.);
    if (n > 0) LSA_TRY(lsa_download_match(Ctx, k, debug[k].status.data(), debug[k].weights.data(), nullptr, n));
  }
  return LSA_OK;
}

// Slam::ComputeEgoMotion (Slam.cxx:813-972)
int SlamCore::ComputeEgoMotion()
{
  Tick tpre;
  Trelative = Pose::Identity();
  if (AheadStatus < 0) { const int rc = AheadStatus; AheadStatus = 0; return Fail(rc, "lsa_prepare_previous_targets (look-ahead thread)"); }
  if (LogTrajectory.size() >= 2 &&
      (EgoMotion == EgoMotionMode::MOTION_EXTRAPOLATION || EgoMotion == EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION))
  {
    const double t = StampToSec(CurrentStamp);
    const double t1 = LogTrajectory[LogTrajectory.size() - 1].time;
    const double t0 = LogTrajectory[LogTrajectory.size() - 2].time;
    if (!(std::abs((t - t1) / (t1 - t0)) > MaxExtrapolationRatio))
    {
      const Pose next = LinearInterpolation(PreviousTworld, Tworld, t, t0, t1);
      Trelative = Inverse(Tworld) * next;
    }
  }
  const bool registers = EgoMotion == EgoMotionMode::REGISTRATION || EgoMotion == EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION;
  {
    const int rc = BeginSubMapSpeculation(Tworld * Trelative);
    if (rc < 0) return rc;
    HoldLookahead = false;  // (from here on DevSpecRunning says whether the speculation is still being enqueued)
  }
  if (!registers) return LSA_OK;

  // kd-trees on the previous frame's raw keypoints -> device search grids, no PCIe traffic
  for (int k : {LSA_EDGE, LSA_PLANE})
  {
    lsa_set_target_cell_size(Ctx, LSA_TARGET_PREVIOUS, k, static_cast<float>(k == LSA_EDGE ? KnnCellSizeEgoMotionEdges : KnnCellSizeEgoMotion));
    LSA_TRY(lsa_set_target_from_set(Ctx, LSA_TARGET_PREVIOUS, k, LSA_SET_RAW_PREVIOUS));
  }
  IcpLoopSpec spec = {};
  spec.name = "ego";
  spec.target = LSA_TARGET_PREVIOUS;
  spec.set = LSA_SET_RAW_CURRENT;
  spec.matchMask = spec.solveMask = (1u << LSA_EDGE) | (1u << LSA_PLANE);
  spec.maxIter = EgoMotionICPMaxIter;
  spec.lmMaxIter = EgoMotionLMMaxIter;
  spec.initSaturation = EgoMotionInitSaturationDistance;
  spec.finalSaturation = EgoMotionFinalSaturationDistance;
  spec.match = EgoMatchParams();
  spec.loopBit = 1;
  spec.linksOk = true;
  spec.matchSerial = EgoMatchSerial;
  spec.icpSeconds = &FrameStats::ego_icp;
  spec.lmSeconds = &FrameStats::ego_lm;
  spec.iterations = &FrameStats::ego_iters;
  spec.countSkippedEvals = true;
  auto enqueued = [&](unsigned icpIter) -> int {
    // the targets of the NEXT frame's ego-motion, which are this frame's keypoints, are built beside this registration:
    // enqueued (ten launches and two copies on the look-ahead stream: a host thread of their own issues them, this one
    // goes on to the solve) while the first iteration's kernels -- the solve's included -- are on their way
    if (icpIter == 0 && BuildTargetsAhead)
    {
      AheadStatus = 0;
      AheadWorker.Submit([this] { AheadStatus = PrepareNextEgoMotionTargets(); });
    }
    // while the device is busy with this iteration: sub-maps the workers have finished meanwhile go to the device
    if (!SpecPending) LSA_TRY(StageSpeculativeSubMaps());
    return LSA_OK;
  };
  // the predicted bounding boxes have long arrived: the map workers extract the sub-maps from here on
  auto solved = [&]() -> int { return SpecPending ? FinishSubMapSpeculation() : LSA_OK; };
  DbgAcc[2] += tpre.Stop();
  // ("Not enough keypoints, EgoMotion skipped for this frame." leaves Trelative as it is)
  if (const int rc = RunIcpLoop(spec, Trelative, kNothing, enqueued, solved, kNothing, kNothing, kNothing); rc < 0) return rc;
  if (KeepMatchDebug) return DownloadMatchDebug(LSA_SET_RAW_CURRENT, spec.matchMask, EgoDebug);
  return LSA_OK;
}

// Slam::Localization (Slam.cxx:975-1175)
int SlamCore::Localization()
{
  Tick tloc;
  struct AtExit { SlamCore* c; Tick* t; ~AtExit() { c->DbgAcc[5] += t->Stop() - (c->Stats.loc_icp + c->Stats.loc_lm + c->Stats.submap + c->Stats.undistort); } } atExit{this, &tloc};
  // the sensor terms enter this frame's localization problem only (Slam.cxx:1123-1131): every solve and the registration
  // error below; cleared on every way out, so that neither the next ego-motion nor anything else sees them
  const bool sensorTerms = LocSensorTerms.wheel || LocSensorTerms.gravity;
  if (sensorTerms) lsa_set_sensor_terms(Ctx, &LocSensorTerms);
  struct SensorTermsGuard { lsa_ctx* ctx; bool on; ~SensorTermsGuard() { if (on) lsa_set_sensor_terms(ctx, nullptr); } } sensorGuard{Ctx, sensorTerms};
  PreviousTworld = Tworld;
  Tworld = PreviousTworld * Trelative;
  // With the maps on the device the reset, the first undistortion and the keypoints' boxes under the pose guess (which the
  // grids read on the device) are one launch; otherwise the three steps as the reference lists them.
  const bool oneLaunch = LocalizationStartFused && DeviceMapsInUse() && MapUpdate != MappingMode::NONE;
  bool boxesEnqueued = false;
  if (oneLaunch)
  {
    Tick t;
    Pose d0 = Pose::Identity(), d1 = Pose::Identity();
    if (Undistortion)
    {
      double t0, t1;
      LSA_TRY(lsa_keypoint_time_range(Ctx, LSA_SET_RAW_CURRENT, &t0, &t1));  // what the working keypoints are about to be
      InitUndistortion(t0, t1);
      RefineUndistortion(&d0, &d1);
    }
    LSA_TRY(lsa_localization_begin(Ctx, Undistortion ? d0.m : nullptr, Undistortion ? d1.m : nullptr, Motion.Time0, Motion.Time1, Tworld.m));
    boxesEnqueued = true;
    Stats.undistort += t.Stop();
  }
  else
  {
    LSA_TRY(lsa_reset_working_keypoints(Ctx));  // CurrentUndistortedKeypoints = CurrentRawKeypoints
    if (Undistortion)
    {
      Tick t;
      int rc = InitUndistortion();
      if (rc < 0) return rc;
      rc = RefineUndistortion();
      if (rc < 0) return rc;
      Stats.undistort += t.Stop();
    }
  }
  // the targets: the sub-maps of the maps as the last keyframe left them (lsa_slam_maps.cpp)
  if (const int rc = PrepareLocalizationSubMaps(boxesEnqueued); rc < 0) return rc;

  const bool refined = Undistortion == UNDISTORTION_REFINED;
  IcpLoopSpec spec = {};
  spec.name = "loc";
  spec.target = LSA_TARGET_MAP;
  spec.set = LSA_SET_WORKING;
  spec.matchMask = UsedTypesMask();
  spec.solveMask = 7u;
  spec.maxIter = LocalizationICPMaxIter;
  spec.lmMaxIter = LocalizationLMMaxIter;
  spec.initSaturation = LocalizationInitSaturationDistance;
  spec.finalSaturation = LocalizationFinalSaturationDistance;
  spec.match = LocMatchParams();
  spec.loopBit = 2;
  // The undistortion between two iterations has to ride in the next search kernel for an iteration to be enqueued ahead (a
  // launch of its own would have to be enqueued between the two, when the motion is known); behind a link the device
  // refines it itself.
  spec.linksOk = !refined || UndistortInSearch;
  spec.undistortAhead = refined ? 1 : 0;
  spec.link.refine_undistortion = refined ? 1 : 0;
  spec.link.have_log = LogTrajectory.empty() ? 0 : 1;
  spec.link.prev_time = LogTrajectory.empty() ? 0. : LogTrajectory.back().time;
  spec.link.cur_time = StampToSec(CurrentStamp);
  spec.link.max_extrapolation_ratio = MaxExtrapolationRatio;
  std::memcpy(spec.link.previous_world, PreviousTworld.m, sizeof(spec.link.previous_world));
  {
    double* m = spec.link.motion;
    m[0] = Motion.Time0; m[1] = Motion.Time1;
    m[2] = Motion.Rot0.w; m[3] = Motion.Rot0.x; m[4] = Motion.Rot0.y; m[5] = Motion.Rot0.z;
    m[6] = Motion.Rot1.w; m[7] = Motion.Rot1.x; m[8] = Motion.Rot1.y; m[9] = Motion.Rot1.z;
    for (int i = 0; i < 3; ++i) { m[10 + i] = Motion.Trans0[i]; m[13 + i] = Motion.Trans1[i]; }
  }
  spec.matchSerial = LocMatchSerial;
  spec.icpSeconds = &FrameStats::loc_icp;
  spec.lmSeconds = &FrameStats::loc_lm;
  spec.iterations = &FrameStats::loc_iters;
  spec.countSkippedEvals = false;
  auto top = [&](unsigned icpIter) -> int {
    // the keyframe's insertion is handed to the maps' thread right after this loop: awake by then (last iteration: ~0.1 ms ahead)
    if (WorkerPrewake && DeviceMapsInUse() && icpIter + 1 == LocalizationICPMaxIter && MapUpdate != MappingMode::NONE) MapWorker[0].Expect(300e-6);
    return LSA_OK;
  };
  auto skipped = [&]() -> int {
    // reset state to previous one to avoid instability (Slam.cxx:1098-1107)
    Trelative = Pose::Identity();
    Tworld = PreviousTworld;
    if (Undistortion) Motion.SetTransforms(Pose::Identity(), Pose::Identity());
    LastError = "Not enough keypoints matched, Localization skipped for this frame.";
    return LSA_OK;
  };
  auto accepted = [&](bool last, IcpUndistortion& undistortion) -> int {
    Trelative = Inverse(PreviousTworld) * Tworld;
    if (!refined) return LSA_OK;
    if (UndistortInSearch && !last)
    {
      undistortion.pending = true;
      return RefineUndistortion(&undistortion.d0, &undistortion.d1);
    }
    return RefineUndistortion();
  };
  auto finished = [&](LocalOptimizer& optimizer) -> int {
    Tick terr;
    LSA_TRY(optimizer.EstimateRegistrationError(LocalizationUncertainty));
    DbgAcc[4] += terr.Stop();
    return LSA_OK;
  };
  if (const int rc = RunIcpLoop(spec, Tworld, top, kNothing, kNothing, skipped, accepted, finished); rc < 0) return rc;
  if (KeepMatchDebug) return DownloadMatchDebug(LSA_SET_WORKING, 7u, LocDebug);
  return LSA_OK;
}

// Slam::InterpolateScanPose (Slam.cxx:1271-1285)
Pose SlamCore::InterpolateScanPose(double time) const
{
  if (LogTrajectory.empty()) return Tworld;
  const double prevPoseTime = LogTrajectory.back().time;
  const double currPoseTime = StampToSec(CurrentStamp);
  if (std::abs(time / (currPoseTime - prevPoseTime)) > MaxExtrapolationRatio) return Tworld;
  return LinearInterpolation(PreviousTworld, Tworld, currPoseTime + time, prevPoseTime, currPoseTime);
}

// Slam::InitUndistortion (Slam.cxx:1288-1319)
int SlamCore::InitUndistortion()
{
  double t0, t1;
  LSA_TRY(lsa_working_time_range(Ctx, &t0, &t1));
  InitUndistortion(t0, t1);
  return LSA_OK;
}
void SlamCore::InitUndistortion(double t0, double t1)
{
  Motion.SetTimes(t0, t1);
  Motion.SetTransforms(Pose::Identity(), Pose::Identity());
  if (Motion.GetTimeRange() < 1e-6) Motion.SetTimes(0., 0.);
}

// Slam::RefineUndistortion (Slam.cxx:1322-1352); with d0 / d1 the two transforms are handed back instead of applied
int SlamCore::RefineUndistortion(Pose* outD0, Pose* outD1)
{
  const Pose previousBaseBegin = Motion.GetH0();
  const Pose previousBaseEnd = Motion.GetH1();
  const Pose worldToBaseBegin = InterpolateScanPose(Motion.Time0);
  const Pose worldToBaseEnd = InterpolateScanPose(Motion.Time1);
  const Pose baseToWorld = Inverse(Tworld);
  const Pose newBaseBegin = baseToWorld * worldToBaseBegin;
  const Pose newBaseEnd = baseToWorld * worldToBaseEnd;
  Motion.SetTransforms(newBaseBegin, newBaseEnd);
  const Pose d0 = newBaseBegin * Inverse(previousBaseBegin);
  const Pose d1 = newBaseEnd * Inverse(previousBaseEnd);
  if (outD0 && outD1) { *outD0 = d0; *outD1 = d1; return LSA_OK; }
  LSA_TRY(lsa_undistort(Ctx, d0.m, d1.m, Motion.Time0, Motion.Time1));
  return LSA_OK;
}

}  // namespace host
}  // namespace lsa
