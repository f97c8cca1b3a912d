// lsa_slam_core.cpp -- see lsa_slam_core.h: construction, the frame path from AddFrame to the end of ProcessCurrentFrame,
// the look-ahead, the getters.  The ICP loops are in lsa_slam_icp.cpp, the maps in lsa_slam_maps.cpp, the keypoint log and
// its calls in lsa_slam_log.cpp, the parameter table in lsa_slam_params.cpp.
#include "lsa_slam_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

namespace lsa
{
namespace host
{
// Slam::Slam (Slam.cxx:143-161)
SlamCore::SlamCore(int device)
{
  ExtractParams = DefaultExtractParams();
  for (int k = 0; k < 3; ++k) LocalMaps[k] = std::make_shared<RollingGrid>();
  if (const char* e = std::getenv("LSA_ICP_AHEAD")) ICPAhead = std::atoi(e);  // default of the parameter (A/B runs)
  // the plane map takes the largest insertions (tens of thousands of keypoints per keyframe): four host threads
  // keep them shorter than the ego-motion ICP they run beside ("MapAddThreads"; the map is the same for any value)
  LocalMaps[LSA_PLANE]->SetAddThreads(4);
  for (int k = 0; k < 3; ++k) LocalMaps[k]->SetVoxelResolution(10.);
  for (int k = 0; k < 3; ++k) LocalMaps[k]->SetGridSize(50);
  LocalMaps[LSA_EDGE]->SetLeafSize(0.30);
  LocalMaps[LSA_PLANE]->SetLeafSize(0.60);
  LocalMaps[LSA_BLOB]->SetLeafSize(0.30);
  const int rc = lsa_ctx_create(device, &Ctx);
  if (rc != LSA_OK)
  {
    Ctx = nullptr;
    LastError = rc == LSA_E_NO_DEVICE ? "no usable HIP device (there is no CPU fallback)" : "lsa_ctx_create failed";
  }
  else
    for (int k = 0; k < 3; ++k)
    {
      lsa_ctx* ctx = Ctx;
      if (lsa_device_grid_create(ctx, &DevMaps[k]) == LSA_OK)
      {
        // the other parameters start from the same defaults as RollingGrid's (RollingGrid.h:170-212) and follow the same
        // setters afterwards (SetVoxelResolution snaps to the leaf size of the moment on both sides, RollingGrid.cxx:73-88)
        lsa_device_grid_set(DevMaps[k], "LeafSize", LocalMaps[k]->GetLeafSize());
      }
      else DevMaps[k] = nullptr;
      LocalMaps[k]->SetSubMapStorage([ctx, k](std::size_t n) { return lsa_target_staging(ctx, LSA_TARGET_MAP, k, static_cast<int>(n)); });
    }
  Reset();
}

SlamCore::~SlamCore()
{
  if (std::getenv("LSA_STAGE_DEBUG") && DbgFrames > 0)
    std::fprintf(stderr, "[stage debug] per frame, us: garbage+adopt %.1f | wait for the look-ahead thread %.1f | ego-motion before its loop %.1f | after the maps %.1f | registration error %.1f | localization outside its stage timers %.1f | of the first: garbage %.1f, up to the hand-over %.1f (%ld frames)\n",
                 1e6 * DbgAcc[0] / DbgFrames, 1e6 * DbgAcc[1] / DbgFrames, 1e6 * DbgAcc[2] / DbgFrames, 1e6 * DbgAcc[3] / DbgFrames, 1e6 * DbgAcc[4] / DbgFrames, 1e6 * DbgAcc[5] / DbgFrames, 1e6 * DbgAcc[6] / DbgFrames, 1e6 * DbgAcc[7] / DbgFrames, DbgFrames);
  WaitMaps();
  for (auto* g : LoopMaps)
    if (g) lsa_device_grid_destroy(g);
  if (LoopCtx) lsa_ctx_destroy(LoopCtx);
  for (auto* g : DevMaps)
    if (g) lsa_device_grid_destroy(g);
  if (Dense) lsa_dense_map_destroy(Dense);
  if (Ctx) lsa_ctx_destroy(Ctx);
}

namespace
{
// Slam::AddFrames with several frames keeps them in the last slots of the context's frame store
constexpr int kMaxDeviceFrames = 16;
constexpr int kFirstDeviceFrameSlot = 65536 - kMaxDeviceFrames - 1;
}  // namespace

int SlamCore::Fail(int rc, const char* where)
{
  LastError = std::string(where) + ": " + (Ctx ? lsa_last_error(Ctx) : "no context");
  return rc;
}

// Slam::Reset (Slam.cxx:164-210)
void SlamCore::Reset(bool resetLog, bool keepDenseMap)
{
  WaitMaps();
  for (int k = 0; k < 3; ++k) LocalMaps[k]->Reset();
  for (auto* g : DevMaps)
    if (g) lsa_device_grid_reset(g, nullptr);
  if (!keepDenseMap) DropDenseMap("Reset or an applied trajectory");
  KfLastPose = Pose::Identity();
  KfCounter = 0;
  Tworld = PreviousTworld = Trelative = Pose::Identity();
  Motion = WithinFrameMotion();
  LocalizationUncertainty = RegistrationError();
  CurrentStamp = 0;  // the "previous frame" after a reset is an empty cloud with stamp 0
  HaveFrame = false;
  // nothing announced ahead of the reset (HintNextFrame) is taken over after it, no ICP iteration stays enqueued
  NextFrameHinted = false;
  if (Ctx)
  {
    (void)lsa_upload_frame_forget(Ctx);
    (void)lsa_icp_abandon(Ctx);
  }
  if (Ctx)
    for (int s = 0; s < 3; ++s)
      for (int k = 0; k < 3; ++k) lsa_set_keypoints(Ctx, s, k, nullptr, 0);
  for (int k = 0; k < 3; ++k) { EgoDebug[k] = MatchDebug(); LocDebug[k] = MatchDebug(); KeypointCounts[k] = 0; SpecBuilt[k] = false; }
  SpecPending = false;
  for (int k = 0; k < 3; ++k)
  {
    SpecDone[k].store(false);
    SpecStaged[k] = false;
    if (Ctx) (void)lsa_drop_target_ahead(Ctx, LSA_TARGET_MAP, k);  // nothing handed over ahead of time survives a reset
  }
  CurrentFrames.clear();
  for (int k = 0; k < 3; ++k) EgoMatchSerial[k] = LocMatchSerial[k] = 0;
  if (resetLog)
  {
    NbrFrameProcessed = 0;
    LogTrajectory.clear();  // LogCovariances is left alone, as in the reference (Slam.cxx:200-209)
    if (Ctx) (void)lsa_kplog_clear(Ctx);  // LogKeypoints.clear()
    KpLogStopped = false;
  }
}

Pose SlamCore::GetWorldTransform(double* time) const
{
  if (time) *time = LogTrajectory.empty() ? 0. : LogTrajectory.back().time;
  return LogTrajectory.empty() ? Pose::Identity() : LogTrajectory.back().pose;
}

// Slam::GetLatencyCompensatedWorldTransform (Slam.cxx:555-590)
Pose SlamCore::GetLatencyCompensatedWorldTransform(double* time) const
{
  const size_t n = LogTrajectory.size();
  if (time) *time = n ? LogTrajectory.back().time : 0.;
  if (n == 0) return Pose::Identity();
  if (n == 1) return LogTrajectory.back().pose;
  const StampedPose& previous = LogTrajectory[n - 2];
  const StampedPose& current = LogTrajectory[n - 1];
  // timestamps undefined or too close / extrapolation too far: the current pose
  if (std::abs(current.time - previous.time) < 1e-6) return current.pose;
  if (std::abs(Latency / (current.time - previous.time)) > MaxExtrapolationRatio) return current.pose;
  return LinearInterpolation(previous.pose, current.pose, current.time + Latency, previous.time, current.time);
}

// Slam::SetWorldTransformFromGuess (Slam.cxx:490-501)
int SlamCore::SetWorldTransformFromGuess(const Pose& guess)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  Tworld = guess;
  // the ego-motion extrapolation then gives identity, and without current keypoints the next frame skips the
  // ego-motion registration
  PreviousTworld = Tworld;
  for (int k = 0; k < 3; ++k) LSA_TRY(lsa_set_keypoints(Ctx, LSA_SET_RAW_CURRENT, k, nullptr, 0));
  return LSA_OK;
}

// Slam::GetDebugInformation (Slam.cxx:610-633)
int SlamCore::GetDebugInformation(double out[10])
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  for (int i = 0; i < 10; ++i) out[i] = 0.;
  int hist[LSA_MATCH_NSTATUS];
  for (int k = 0; k < 3; ++k)
  {
    // MatchingResults::NbMatches() = RejectionsHistogram[SUCCESS] of the last iteration's match
    if (k < 2 && EgoMatchSerial[k] > 0)
    {
      LSA_TRY(lsa_match_histogram(Ctx, k, EgoMatchSerial[k], hist));
      out[k] = hist[LSA_MATCH_SUCCESS];
    }
    if (LocMatchSerial[k] > 0)
    {
      LSA_TRY(lsa_match_histogram(Ctx, k, LocMatchSerial[k], hist));
      out[2 + k] = hist[LSA_MATCH_SUCCESS];
    }
  }
  out[5] = LocalizationUncertainty.PositionError;
  out[6] = LocalizationUncertainty.OrientationError;
  out[7] = OverlapEstimation;
  out[8] = ComplyMotionLimits ? 1. : 0.;
  out[9] = Latency;
  return LSA_OK;
}

// Slam::AddFrames (Slam.cxx:230-344) + CheckFrames (:709-743)
int SlamCore::AddFrame(const lsa_point_t* pts, int n, uint64_t stampUs, uint32_t)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  Tick total;
  Stats = FrameStats();
  (void)lsa_collect_garbage(Ctx);  // buffers outgrown during the last frame (nothing on the device waits for the host here)
  DbgAcc[6] += total.Stop();
  if (!pts || n <= 0) { LastError = "SLAM input only contains empty pointclouds : exiting."; return LSA_OK; }
  if (stampUs == CurrentStamp) { LastError = "SLAM frames have the same timestamp as previous ones : frames ignored."; return LSA_OK; }
  if (pts[0].device_id != 0 && (!OtherExtractors.empty() || !OtherBaseToLidarOffsets.empty()))
  {
    // a frame of another device that has an extractor or an offset of its own
    const InputFrame f{pts, n, stampUs, 0};
    return AddFrames(&f, 1);
  }
  CurrentFrames.clear();
  DbgAcc[7] += total.Stop();
  {
    // the cloud may have been announced and uploaded ahead (HintNextFrame): it is taken over, otherwise copied now
    const int adopted = lsa_upload_frame_adopt(Ctx, pts, n);
    if (adopted < 0) return Fail(adopted, "lsa_upload_frame_adopt");
    if (adopted == 0) LSA_TRY(lsa_upload_frame(Ctx, pts, n));
  }
  if (NbrFrameProcessed == 8) { for (double& d : DbgAcc) d = 0.; DbgFrames = 0; }  // (the first frames allocate)
  DbgAcc[0] += total.Stop();
  DbgFrames++;
  int rc = ProcessCurrentFrame(stampUs);
  Latency = Stats.total = total.Stop();
  return rc;
}

int SlamCore::AddStoredFrame(int slot, uint64_t stampUs, uint32_t)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  Tick total;
  Stats = FrameStats();
  if (stampUs == CurrentStamp) { LastError = "SLAM frames have the same timestamp as previous ones : frames ignored."; return LSA_OK; }
  CurrentFrames.clear();
  LSA_TRY(lsa_frame_store_use(Ctx, slot));
  int rc = ProcessCurrentFrame(stampUs);
  Latency = Stats.total = total.Stop();
  return rc;
}

int SlamCore::HintNextFrame(const lsa_point_t* pts, int n)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (!pts || n <= 0) return LSA_OK;
  NextFrameHinted = false;
  LSA_TRY(lsa_upload_frame_begin(Ctx, pts, n));
  NextFrameHinted = true;
  return LSA_OK;
}

// The look-ahead extraction of the cloud announced with HintNextFrame starts as soon as (i) the current frame's own
// extraction is over and (ii) the uploader thread has enqueued the DMA: asked for after the extraction and between
// the steps of the ICP loops.
int SlamCore::TryStartLookahead()
{
  // (not while the sub-maps ahead of time are still being enqueued on the same stream: ProcessCurrentFrame)
  if (!NextFrameHinted || HoldLookahead || DevSpecRunning.load(std::memory_order_acquire) || !lsa_upload_frame_ready(Ctx)) return LSA_OK;
  NextFrameHinted = false;
  if (lsa_extract_prefetch_uploaded(Ctx, &ExtractParams) != LSA_OK) LastError = std::string("look-ahead ignored: ") + lsa_last_error(Ctx);
  return LSA_OK;
}

// The next frame's extraction (a dozen launches on the look-ahead stream once its upload has arrived) is enqueued by this
// thread between the launch of a solve and the wait for its result, not between the match and the solve: the solve's
// kernel then follows the model fits at once (it came 56 us late whenever the look-ahead was enqueued in front of it).
void SlamCore::ArmLookaheadInterlude()
{
  InterludeRan = false;
  InterludeStatus = LSA_OK;
  if (!DeviceLM) return;  // the host-driven loop has no such gap: FinishLookaheadInterlude does the work
  lsa_solve_device_interlude(Ctx, [](void* self) {
    SlamCore* core = static_cast<SlamCore*>(self);
    core->InterludeStatus = core->InterludeWork();
    core->InterludeRan = true;
  }, this);
}
int SlamCore::FinishLookaheadInterlude()
{
  if (DeviceLM) lsa_solve_device_interlude(Ctx, nullptr, nullptr);  // a solve that never got to its launch leaves it armed
  if (!InterludeRan) InterludeStatus = InterludeWork();
  InterludeRan = true;
  return InterludeStatus;
}
// what this thread enqueues while a solve runs: the next frame's extraction once its upload is there, and (once per frame,
// with the first solve of the ego-motion ICP) the sub-maps for the predicted boxes on the device
int SlamCore::InterludeWork()
{
  LSA_TRY(TryStartLookahead());
  return LSA_OK;
}

// Slam::AddFrames with several frames, one per LiDAR device (Slam.cxx:230-344; CheckFrames :709-743)
int SlamCore::AddFrames(const InputFrame* frames, int nframes)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (!frames || nframes <= 0 || nframes > kMaxDeviceFrames) { LastError = "AddFrames: between 1 and 16 frames"; return LSA_E_ARG; }
  // one frame of the default device with nothing configured per device: the plain path (no device-resident copy)
  const bool perDevice = !OtherExtractors.empty() || !OtherBaseToLidarOffsets.empty();
  if (nframes == 1 && (!frames[0].pts || frames[0].n <= 0 || frames[0].pts[0].device_id == 0 || !perDevice))
    return AddFrame(frames[0].pts, frames[0].n, frames[0].stampUs, frames[0].seq);
  Tick total;
  Stats = FrameStats();
  (void)lsa_collect_garbage(Ctx);
  bool allEmpty = true;
  for (int i = 0; i < nframes; ++i)
    if (frames[i].pts && frames[i].n > 0) allEmpty = false;
  if (allEmpty) { LastError = "SLAM input only contains empty pointclouds : exiting."; return LSA_OK; }
  if (frames[0].stampUs == CurrentStamp) { LastError = "SLAM frames have the same timestamp as previous ones : frames ignored."; return LSA_OK; }
  // the frames become device-resident: the extraction, the registered frame and the overlap estimator read them
  CurrentFrames.clear();
  Device0AzimuthalResolution = lsa_get_azimuthal_resolution(Ctx);
  for (int i = 0; i < nframes; ++i)
  {
    if (!frames[i].pts || frames[i].n <= 0) continue;  // "SLAM input frame i is an empty pointcloud : frame ignored."
    const int device = frames[i].pts[0].device_id;
    // the azimuthal resolution is estimated from a device's first frame while it is handed over
    float* az = device == 0 ? &Device0AzimuthalResolution : (OtherExtractors.count(device) ? &OtherExtractors[device].azimuthalResolution : nullptr);
    if (!az && OtherExtractors.empty()) az = &Device0AzimuthalResolution;  // the default extractor stands in (Slam.cxx:766-772)
    lsa_set_azimuthal_resolution(Ctx, az ? *az : 1.f);
    const int slot = kFirstDeviceFrameSlot + i;
    if (lsa_frame_store_put(Ctx, slot, frames[i].pts, frames[i].n) != LSA_OK)
    {
      lsa_set_azimuthal_resolution(Ctx, Device0AzimuthalResolution);  // device 0's value goes back where it lives
      CurrentFrames.clear();
      return Fail(LSA_E_HIP, "AddFrames");
    }
    if (az) *az = lsa_get_azimuthal_resolution(Ctx);
    CurrentFrames.push_back({slot, frames[i].n, device, StampToSec(frames[i].stampUs) - StampToSec(frames[0].stampUs)});
  }
  lsa_set_azimuthal_resolution(Ctx, Device0AzimuthalResolution);
  int rc = ProcessCurrentFrame(frames[0].stampUs);
  Latency = Stats.total = total.Stop();
  return rc;
}

void SlamCore::ApplySearchTuning(lsa_ctx* ctx)
{
  lsa_set_knn_lanes(ctx, LSA_EDGE, KnnLanesEdges);
  lsa_set_knn_lanes(ctx, LSA_PLANE, KnnLanesPlanes);
  lsa_set_knn_lanes(ctx, LSA_BLOB, KnnLanesBlobs);
  lsa_set_knn_rounds(ctx, LSA_EDGE, KnnRoundsEdges);
  lsa_set_knn_rounds(ctx, LSA_PLANE, KnnRoundsPlanes);
  lsa_set_knn_rounds(ctx, LSA_BLOB, KnnRoundsBlobs);
  lsa_set_fused_match(ctx, FusedMatch ? 1 : 0);
}

int SlamCore::ProcessCurrentFrame(uint64_t stampUs)
{
  CurrentStamp = stampUs;
  CurrentTime = StampToSec(stampUs);
  HaveFrame = true;
  DenseLastOrdinal = -1;  // the current frame changes here: it is in the dense map only once InsertDenseFrame has put it there
  {
    Tick t;
    AheadWorker.Wait();  // it reads the previous frame's keypoint buffers, which the extraction is about to rotate (long done)
    DbgAcc[1] += t.Stop();
  }
  // The look-ahead stream carries, in this order of urgency: the previous keyframe's insertion and the sub-maps extracted
  // ahead of time (this frame's localization waits for them), the next frame's ego-motion targets, the next frame's
  // extraction (nobody waits for it before the next AddFrame).  An upload that is there early must not put the extraction in
  // front: with the cloud staged by four threads the sub-map stage went from 0.02 to 0.12 ms per frame (1 250 -> 1 100 frames/s).
  // Held back until the speculation has been enqueued (BeginSubMapSpeculation, DevSpecRunning).
  HoldLookahead = DeviceMapsInUse() && SubMapsAhead && MapUpdate != MappingMode::NONE;
  ApplySearchTuning(Ctx);
  {
    Tick t;
    int rc = ExtractKeypoints();
    if (rc < 0) return rc;
    Stats.extract = t.Stop();
  }
  int rc = ComputeEgoMotion();
  if (rc < 0) return rc;
  // Slam::ComputeSensorConstraints (Slam.cxx:256-261): the managers compute at the first frame's time when either one is
  // usable; otherwise the previous frame's terms stay, with their weights
  LocSensorTerms = SensorManagers.Compute(CurrentTime);
  rc = Localization();
  if (rc < 0) return rc;
  Tick tail;
  // confidence estimators: before the maps update, which invalidates the sub-maps (Slam.cxx:269-280)
  if (OverlapSamplingRatio > 0)
  {
    rc = EstimateOverlap();
    if (rc < 0) return rc;
  }
  if (TimeWindowDuration > 0) CheckMotionLimits();
  const int keyframesBefore = KfCounter;
  if (MapUpdate == MappingMode::ADD_KPTS_TO_FIXED_MAP || MapUpdate == MappingMode::UPDATE)
  {
    Tick t;
    rc = UpdateMapsUsingTworld();
    if (rc < 0) return rc;
    Stats.maps = t.Stop();
  }
  // the words the next frame's localization reduces its keypoints' boxes into, armed while the device has nothing to do
  if (LocalizationStartFused && DeviceMapsInUse() && MapUpdate != MappingMode::NONE) LSA_TRY(lsa_arm_localization_boxes(Ctx));
  LogCurrentFrameState(CurrentTime);
  // Tworld and the motion within the frame are final: the registered frame goes into the dense map (off: nothing)
  if (DenseMapMode != 0)
  {
    rc = InsertDenseFrame(KfCounter != keyframesBefore, CurrentTime);
    if (rc < 0) return rc;
  }
  // the next frame's first jobs for the look-ahead thread (the sub-maps under the predicted pose, the ego-motion targets) come
  // within a fraction of a millisecond when the caller replays: the thread is awake for them
  if (WorkerPrewake && DeviceMapsInUse()) AheadWorker.Expect(300e-6);
  NbrFrameProcessed++;
  DbgAcc[3] += tail.Stop() - Stats.maps;
  return LSA_OK;
}

// Slam::ExtractKeypoints (Slam.cxx:746-810)
int SlamCore::ExtractKeypoints()
{
  int counts[3];
  lsa_set_keypoint_types(Ctx, UsedTypesMask());  // unused types come out empty (Slam.cxx:789-793)
  if (!CurrentFrames.empty()) return ExtractFrames();
  LSA_TRY(lsa_extract_keypoints(Ctx, &ExtractParams, counts));  // also: PreviousRawKeypoints = CurrentRawKeypoints
  for (int k = 0; k < 3; ++k) KeypointCounts[k] = counts[k];
  // AggregateFrames(keypoints, false): LIDAR -> BASE (Slam.cxx:1551-1573); skipped when identity
  if (!IsApprox(BaseToLidarOffset, Pose::Identity()))
    for (int k = 0; k < 3; ++k)
      if (counts[k] > 0) LSA_TRY(lsa_transform_keypoints(Ctx, LSA_SET_RAW_CURRENT, k, BaseToLidarOffset.m, 0.));
  if (NextStoredSlot >= 0)
  {
    // look-ahead: the next frame's extraction runs on its own stream beside this frame's registration; a slot that
    // does not exist is reported and otherwise ignored
    if (lsa_extract_prefetch(Ctx, NextStoredSlot, &ExtractParams) != LSA_OK) LastError = std::string("look-ahead ignored: ") + lsa_last_error(Ctx);
    NextStoredSlot = -1;
  }
  LSA_TRY(TryStartLookahead());
  return LSA_OK;
}

// Slam::ExtractKeypoints with several device frames (Slam.cxx:753-801) + AggregateFrames(keypoints, false) (:1512-1578)
int SlamCore::ExtractFrames()
{
  for (int k = 0; k < 3; ++k) KeypointCounts[k] = 0;
  bool first = true;
  for (const HeldFrame& f : CurrentFrames)
  {
    // the extractor of the frame's device; with a single extractor configured, that one stands in (Slam.cxx:762-779)
    const lsa_extract_params_t* params = nullptr;
    float* az = nullptr;
    if (f.device == 0) { params = &ExtractParams; az = &Device0AzimuthalResolution; }
    else if (OtherExtractors.count(f.device)) { params = &OtherExtractors[f.device].params; az = &OtherExtractors[f.device].azimuthalResolution; }
    else if (OtherExtractors.empty()) { params = &ExtractParams; az = &Device0AzimuthalResolution; }
    else
    {
      LastError = "Input frame comes from LiDAR device " + std::to_string(f.device) + " but no keypoints extractor has been set for this device : ignoring frame.";
      continue;
    }
    LSA_TRY(lsa_frame_store_use(Ctx, f.slot));
    lsa_set_azimuthal_resolution(Ctx, *az);
    // the offset is looked up by the device the points say they come from (Slam.cxx:1540)
    const Pose offset = GetBaseToLidarOffset(f.device);
    const bool identity = IsApprox(offset, Pose::Identity());
    int counts[3] = {0, 0, 0};
    if (first)
    {
      LSA_TRY(lsa_extract_keypoints(Ctx, params, counts));  // also: PreviousRawKeypoints = CurrentRawKeypoints
      if (!identity || f.timeOffset != 0.)
        for (int k = 0; k < 3; ++k)
          if (counts[k] > 0) LSA_TRY(lsa_transform_keypoints(Ctx, LSA_SET_RAW_CURRENT, k, offset.m, f.timeOffset));
    }
    else
      LSA_TRY(lsa_extract_keypoints_more(Ctx, params, identity ? nullptr : offset.m, f.timeOffset, counts));
    first = false;
    for (int k = 0; k < 3; ++k) KeypointCounts[k] += counts[k];
  }
  lsa_set_azimuthal_resolution(Ctx, Device0AzimuthalResolution);
  if (first)
    // no frame had an extractor: the current keypoints are empty (the previous ones are not consulted then)
    for (int k = 0; k < 3; ++k) LSA_TRY(lsa_set_keypoints(Ctx, LSA_SET_RAW_CURRENT, k, nullptr, 0));
  return LSA_OK;
}

// The kd-trees ComputeEgoMotion builds on the previous frame's keypoints (Slam.cxx:845-860) only depend on this
// frame's keypoints: their device counterparts are built now, beside this frame's registration, and found ready by
// the next frame.
int SlamCore::PrepareNextEgoMotionTargets()
{
  if (!BuildTargetsAhead) return LSA_OK;
  if (!(EgoMotion == EgoMotionMode::REGISTRATION || EgoMotion == EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION)) return LSA_OK;
  return lsa_prepare_previous_targets(Ctx, (1u << LSA_EDGE) | (1u << LSA_PLANE));
}

// Slam::EstimateOverlap (Slam.cxx:1370-1388): Confidence::LCPEstimator on the registered frame
int SlamCore::EstimateOverlap()
{
  unsigned mask = 0;
  double leaf[3];
  for (int k = 0; k < 3; ++k)
  {
    leaf[k] = LocalMaps[k]->GetLeafSize();
    if (UseKeypoints[k] && (DeviceMapsInUse() ? lsa_target_size(Ctx, LSA_TARGET_MAP, k) > 0 : LocalMaps[k]->IsSubMapValid())) mask |= 1u << k;
  }
  if (!CurrentFrames.empty())
  {
    // several device frames: the estimator samples the aggregated registered cloud (Slam.cxx:1373); it is built
    // once (GetRegisteredFrame) and handed back as one frame of world points
    LSA_TRY(GetRegisteredFrame(Scratch));
    if (Scratch.empty()) { OverlapEstimation = -1.f; return LSA_OK; }
    LSA_TRY(lsa_frame_store_put(Ctx, kFirstDeviceFrameSlot + kMaxDeviceFrames, Scratch.data(), static_cast<int>(Scratch.size())));
    LSA_TRY(lsa_frame_store_use(Ctx, kFirstDeviceFrameSlot + kMaxDeviceFrames));
    const Pose identity = Pose::Identity();
    LSA_TRY(lsa_overlap(Ctx, mask, 0, identity.m, nullptr, 0., 0., OverlapSamplingRatio, leaf, &OverlapEstimation));
    return LSA_OK;
  }
  if (Undistortion)
  {
    const Pose H0 = (Tworld * Motion.GetH0()) * BaseToLidarOffset;
    const Pose H1 = (Tworld * Motion.GetH1()) * BaseToLidarOffset;
    LSA_TRY(lsa_overlap(Ctx, mask, 1, H0.m, H1.m, Motion.Time0, Motion.Time1, OverlapSamplingRatio, leaf, &OverlapEstimation));
  }
  else
  {
    const Pose tf = Tworld * BaseToLidarOffset;
    LSA_TRY(lsa_overlap(Ctx, mask, 0, tf.m, nullptr, 0., 0., OverlapSamplingRatio, leaf, &OverlapEstimation));
  }
  return LSA_OK;
}

// Slam::CheckMotionLimits (Slam.cxx:1391-1484)
void SlamCore::CheckMotionLimits()
{
  const int nPoses = static_cast<int>(LogTrajectory.size());
  if (nPoses == 0) return;
  const double currentTimeStamp = StampToSec(CurrentStamp);
  double deltaTime = currentTimeStamp - LogTrajectory.back().time;
  double nextDeltaTime = std::numeric_limits<float>::max();
  int startIndex = nPoses - 1;  // the window ends on the current pose and starts at this logged one
  if (deltaTime < TimeWindowDuration)
  {
    // an interval [deltaTime, nextDeltaTime] containing TimeWindowDuration
    while (startIndex >= 0)
    {
      deltaTime = nextDeltaTime;
      nextDeltaTime = currentTimeStamp - LogTrajectory[startIndex].time;
      if (nextDeltaTime >= TimeWindowDuration) break;
      --startIndex;
    }
    if (startIndex < 0) startIndex = 0;  // not enough logged poses: the oldest one
    else if (std::abs(deltaTime - TimeWindowDuration) < std::abs(nextDeltaTime - TimeWindowDuration)) ++startIndex;
    deltaTime = currentTimeStamp - LogTrajectory[startIndex].time;
  }
  ComplyMotionLimits = true;
  const Pose window = Inverse(LogTrajectory[startIndex].pose) * Tworld;
  float angle = static_cast<float>(RotationAngle(window));  // [0, 2 pi]
  if (angle > M_PI) angle = static_cast<float>(2 * M_PI - angle);
  angle = static_cast<float>(angle / M_PI * 180.);  // Utils::Rad2Deg (Utilities.h:150-153)
  const float distance = static_cast<float>(std::sqrt(window.m[3] * window.m[3] + window.m[7] * window.m[7] + window.m[11] * window.m[11]));
  const float velocity[2] = {static_cast<float>(distance / deltaTime), static_cast<float>(angle / deltaTime)};
  if (NbrFrameProcessed >= 2)
  {
    bool comply = true;
    for (int i = 0; i < 2; ++i)
    {
      // Eigen::Array2f / double: the scalar is converted to the array's type first
      const float acceleration = (velocity[i] - PreviousVelocity[i]) / static_cast<float>(deltaTime);
      comply = comply && velocity[i] < VelocityLimits[i] && std::abs(acceleration) < AccelerationLimits[i];
    }
    ComplyMotionLimits = comply;
  }
  PreviousVelocity[0] = velocity[0];
  PreviousVelocity[1] = velocity[1];
  if (!ComplyMotionLimits) LastError = "The pose does not comply with the motion limitations. Lidar SLAM may have failed.";
}

int SlamCore::GetKeypoints(int type, bool world, std::vector<lsa_point_t>& out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const int n = lsa_keypoint_count(Ctx, LSA_SET_WORKING, type);
  out.resize(std::max(n, 0));
  if (n <= 0) return 0;
  if (world) LSA_TRY(lsa_download_transformed(Ctx, LSA_SET_WORKING, type, Tworld.m, out.data(), n));
  else LSA_TRY(lsa_download_keypoints(Ctx, LSA_SET_WORKING, type, out.data(), n));
  return n;
}

int SlamCore::GetRawKeypoints(int type, std::vector<lsa_point_t>& out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const int n = lsa_keypoint_count(Ctx, LSA_SET_RAW_CURRENT, type);
  out.resize(std::max(n, 0));
  if (n > 0) LSA_TRY(lsa_download_keypoints(Ctx, LSA_SET_RAW_CURRENT, type, out.data(), n));
  return n;
}

// Slam::GetRegisteredFrame -> AggregateFrames(CurrentFrames, true) (Slam.cxx:660-667, 1512-1578)
int SlamCore::GetRegisteredFrame(std::vector<lsa_point_t>& out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  out.clear();
  if (!HaveFrame) return 0;
  if (!CurrentFrames.empty())
  {
    // AggregateFrames(CurrentFrames, true): every device frame with its own offset and time shift (Slam.cxx:1512-1578)
    size_t total = 0;
    for (const HeldFrame& f : CurrentFrames) total += static_cast<size_t>(f.n);
    out.resize(total);
    size_t at = 0;
    for (const HeldFrame& f : CurrentFrames)
    {
      LSA_TRY(lsa_frame_store_use(Ctx, f.slot));
      const Pose offset = GetBaseToLidarOffset(f.device);
      if (Undistortion)
      {
        const Pose H0 = (Tworld * Motion.GetH0()) * offset;
        const Pose H1 = (Tworld * Motion.GetH1()) * offset;
        LSA_TRY(lsa_transform_frame_at(Ctx, 1, H0.m, H1.m, Motion.Time0, Motion.Time1, f.timeOffset, out.data() + at, f.n));
      }
      else
      {
        const Pose tf = Tworld * offset;
        LSA_TRY(lsa_transform_frame_at(Ctx, 0, tf.m, nullptr, 0., 0., f.timeOffset, out.data() + at, f.n));
      }
      at += static_cast<size_t>(f.n);
    }
    return static_cast<int>(total);
  }
  const int n = lsa_frame_size(Ctx);
  if (n <= 0) return 0;
  out.resize(n);
  if (Undistortion)
  {
    const Pose H0 = (Tworld * Motion.GetH0()) * BaseToLidarOffset;
    const Pose H1 = (Tworld * Motion.GetH1()) * BaseToLidarOffset;
    LSA_TRY(lsa_transform_frame(Ctx, 1, H0.m, H1.m, Motion.Time0, Motion.Time1, out.data(), n));
  }
  else
  {
    // the reference skips the work when the transform is identity; applying identity gives the same points
    const Pose tf = Tworld * BaseToLidarOffset;
    LSA_TRY(lsa_transform_frame(Ctx, 0, tf.m, nullptr, 0., 0., out.data(), n));
  }
  return n;
}

}  // namespace host
}  // namespace lsa
