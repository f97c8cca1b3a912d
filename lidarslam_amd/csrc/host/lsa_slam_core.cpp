// lsa_slam_core.cpp -- see lsa_slam_core.h.
#include "lsa_slam_core.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <ctime>
#include "lsa_pcd.h"
#include "../lsa_device_grid_io.h"
#include "../lsa_kplog_io.h"
#include "lsa_pose_graph.h"

namespace lsa
{
namespace host
{
constexpr unsigned kChainMax = 6;  // ICP iterations of one loop enqueued at once behind links (lsa_icp_link: 7 blocks, 7 mailboxes)
namespace
{
#define ICP_TRACE(...) do { if (lsa_icp_trace_on()) std::fprintf(stderr, __VA_ARGS__); } while (0)
struct Tick
{
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double Stop() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
inline double StampToSec(uint64_t us) { return us * 1e-6; }  // Utils::PclStampToSec
}  // namespace

static long long SteadyNs() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
HostWorker::HostWorker() : T([this] { Run(); }) {}
HostWorker::~HostWorker()
{
  {
    std::lock_guard<std::mutex> l(M);
    Quit = true;
    Leaving.store(true);
  }
  Cv.notify_all();
  T.join();
}
void HostWorker::Submit(std::function<void()> job)
{
  {
    std::lock_guard<std::mutex> l(M);
    Jobs.push_back(std::move(job));
    Posted.fetch_add(1, std::memory_order_release);
  }
  Cv.notify_one();
}
void HostWorker::Expect(double seconds)
{
  PollUntil.store(SteadyNs() + static_cast<long long>(seconds * 1e9), std::memory_order_release);
  Cv.notify_one();
}
void HostWorker::Wait()
{
  std::unique_lock<std::mutex> l(M);
  Idle.wait(l, [this] { return Jobs.empty() && !Busy; });
}
void HostWorker::Run()
{
  std::unique_lock<std::mutex> l(M);
  while (true)
  {
    Cv.wait(l, [this] { return Quit || !Jobs.empty() || SteadyNs() < PollUntil.load(std::memory_order_acquire); });
    if (Jobs.empty())
    {
      if (Quit) return;  // nothing left to do
      // woken ahead of a job (Expect): poll for it, without the lock, until it is there or the time is up
      l.unlock();
      while (Posted.load(std::memory_order_acquire) == 0 && !Leaving.load() && SteadyNs() < PollUntil.load(std::memory_order_acquire))
      {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
      PollUntil.store(0, std::memory_order_release);
      l.lock();
      continue;
    }
    std::function<void()> job = std::move(Jobs.front());
    Jobs.pop_front();
    Posted.fetch_sub(1, std::memory_order_release);
    Busy = true;
    l.unlock();
    job();
    l.lock();
    Busy = false;
    if (Jobs.empty()) Idle.notify_all();
  }
}

#define LSA_TRY(call)                          \
  do                                           \
  {                                            \
    int rc__ = (call);                         \
    if (rc__ < 0) return Fail(rc__, #call);    \
  } while (0)

// Slam::Slam (Slam.cxx:143-161)
SlamCore::SlamCore(int device)
{
  ExtractParams.neighbor_width = 4;
  ExtractParams.min_distance_to_sensor = 1.5f;
  ExtractParams.min_beam_surface_angle = 10.f;
  ExtractParams.plane_sin_angle_threshold = 0.5f;
  ExtractParams.edge_sin_angle_threshold = 0.86f;
  ExtractParams.dist_to_line_threshold = 0.20f;
  ExtractParams.edge_depth_gap_threshold = 0.15f;
  ExtractParams.edge_saliency_threshold = 1.5f;
  ExtractParams.edge_intensity_gap_threshold = 50.f;
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
  if (Ctx) lsa_ctx_destroy(Ctx);
}

namespace
{
// Slam::AddFrames with several frames keeps them in the last slots of the context's frame store
constexpr int kMaxDeviceFrames = 16;
constexpr int kFirstDeviceFrameSlot = 65536 - kMaxDeviceFrames - 1;

lsa_extract_params_t DefaultExtractParams()
{
  return lsa_extract_params_t{4, 1.5f, 10.f, 0.5f, 0.86f, 0.20f, 0.15f, 1.5f, 50.f};  // SSKE.h:125-148
}
}  // namespace

int SlamCore::Fail(int rc, const char* where)
{
  LastError = std::string(where) + ": " + (Ctx ? lsa_last_error(Ctx) : "no context");
  return rc;
}

// Slam::Reset (Slam.cxx:164-210)
void SlamCore::Reset(bool resetLog)
{
  WaitMaps();
  for (int k = 0; k < 3; ++k) LocalMaps[k]->Reset();
  for (auto* g : DevMaps)
    if (g) lsa_device_grid_reset(g, nullptr);
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

int SlamCore::SetExtractorParam(int deviceId, const std::string& name, double v)
{
  if (deviceId < 0 || deviceId > 255) return LSA_E_ARG;
  if (deviceId == 0) return SetParam(name, v);
  const bool known = OtherExtractors.count(deviceId) != 0;
  DeviceExtractor e = known ? OtherExtractors[deviceId] : DeviceExtractor{DefaultExtractParams(), 0.f};
  lsa_extract_params_t& p = e.params;
  if (name == "NeighborWidth") p.neighbor_width = static_cast<int>(v);
  else if (name == "MinDistanceToSensor") p.min_distance_to_sensor = static_cast<float>(v);
  else if (name == "MinBeamSurfaceAngle") p.min_beam_surface_angle = static_cast<float>(v);
  else if (name == "PlaneSinAngleThreshold") p.plane_sin_angle_threshold = static_cast<float>(v);
  else if (name == "EdgeSinAngleThreshold") p.edge_sin_angle_threshold = static_cast<float>(v);
  else if (name == "EdgeDepthGapThreshold") p.edge_depth_gap_threshold = static_cast<float>(v);
  else if (name == "EdgeSaliencyThreshold") p.edge_saliency_threshold = static_cast<float>(v);
  else if (name == "EdgeIntensityGapThreshold") p.edge_intensity_gap_threshold = static_cast<float>(v);
  else if (name == "AzimuthalResolution") e.azimuthalResolution = static_cast<float>(v);
  else { LastError = "unknown extractor parameter " + name; return LSA_E_ARG; }
  OtherExtractors[deviceId] = e;
  return LSA_OK;
}

int SlamCore::GetExtractorParam(int deviceId, const std::string& name, double* v) const
{
  if (!v) return LSA_E_ARG;
  if (deviceId == 0) return GetParam(name, v);
  const auto it = OtherExtractors.find(deviceId);
  if (it == OtherExtractors.end()) return LSA_E_ARG;
  const lsa_extract_params_t& p = it->second.params;
  if (name == "NeighborWidth") *v = p.neighbor_width;
  else if (name == "MinDistanceToSensor") *v = p.min_distance_to_sensor;
  else if (name == "MinBeamSurfaceAngle") *v = p.min_beam_surface_angle;
  else if (name == "PlaneSinAngleThreshold") *v = p.plane_sin_angle_threshold;
  else if (name == "EdgeSinAngleThreshold") *v = p.edge_sin_angle_threshold;
  else if (name == "EdgeDepthGapThreshold") *v = p.edge_depth_gap_threshold;
  else if (name == "EdgeSaliencyThreshold") *v = p.edge_saliency_threshold;
  else if (name == "EdgeIntensityGapThreshold") *v = p.edge_intensity_gap_threshold;
  else if (name == "AzimuthalResolution") *v = it->second.azimuthalResolution;
  else return LSA_E_ARG;
  return LSA_OK;
}

int SlamCore::SetBaseToLidarOffset(int deviceId, const Pose& offset)
{
  if (deviceId < 0 || deviceId > 255) return LSA_E_ARG;
  if (deviceId == 0) BaseToLidarOffset = offset;
  else OtherBaseToLidarOffsets[deviceId] = offset;
  return LSA_OK;
}

// Slam::GetBaseToLidarOffset (Slam.cxx): identity for a device nobody configured
Pose SlamCore::GetBaseToLidarOffset(int deviceId) const
{
  if (deviceId == 0) return BaseToLidarOffset;
  const auto it = OtherBaseToLidarOffsets.find(deviceId);
  return it == OtherBaseToLidarOffsets.end() ? Pose::Identity() : it->second;
}

int SlamCore::ProcessCurrentFrame(uint64_t stampUs)
{
  CurrentStamp = stampUs;
  CurrentTime = StampToSec(stampUs);
  HaveFrame = true;
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
  lsa_set_knn_lanes(Ctx, LSA_EDGE, KnnLanesEdges);
  lsa_set_knn_lanes(Ctx, LSA_PLANE, KnnLanesPlanes);
  lsa_set_knn_lanes(Ctx, LSA_BLOB, KnnLanesBlobs);
  lsa_set_knn_rounds(Ctx, LSA_EDGE, KnnRoundsEdges);
  lsa_set_knn_rounds(Ctx, LSA_PLANE, KnnRoundsPlanes);
  lsa_set_knn_rounds(Ctx, LSA_BLOB, KnnRoundsBlobs);
  lsa_set_fused_match(Ctx, FusedMatch ? 1 : 0);
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
  unsigned mask = 0;
  for (int k = 0; k < 3; ++k)
    if (UseKeypoints[k]) mask |= 1u << k;
  lsa_set_keypoint_types(Ctx, mask);  // unused types come out empty (Slam.cxx:789-793)
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

  if (DeviceMapsInUse())
  {
    // Slam.cxx:1003-1037 with the maps on the device: a map whose last keyframe changed a point gives a new sub-map --
    // the voxels the box of the current keypoints (at the initial pose guess) touches -- written straight into the
    // target; only the box (read back once for all types) and the sub-maps' sizes cross the bus
    Tick t;
    // the workers have enqueued the previous keyframe's insertions, and the sub-maps ahead of time (NOT the next frame's
    // ego-motion targets, which the look-ahead thread may still be enqueueing: nothing here depends on them)
    for (auto& w : MapWorker) w.Wait();
    {
      // the sub-maps ahead of time: waited for -- and when that took time twice in a row (the ego-motion ICP of this sensor
      // is shorter than insertion + extraction + grid build), not tried again for a while ("SubMapsAheadAdaptive")
      Tick tw;
      while (DevSpecRunning.load(std::memory_order_acquire)) std::this_thread::yield();
      const bool tried = DevSpec[0] || DevSpec[1] || DevSpec[2];
      if (tried && SubMapsAheadAdaptive && tw.Stop() > 80e-6)
      {
        DevSpecGood = 0;
        if (++DevSpecLate >= 2)
        {
          // not tried for a while; twice as long every time it happens again soon (a sensor whose ego-motion ICP is simply
          // too short ends up trying once in 64 frames, an occasional hiccup costs four)
          DevSpecBackoff = DevSpecPenalty;
          DevSpecPenalty = std::min(2 * DevSpecPenalty, 64);
          DevSpecLate = 0;
        }
      }
      else if (tried)
      {
        DevSpecLate = 0;
        if (++DevSpecGood >= 8) DevSpecPenalty = 4;
      }
    }
    Stats.maps_wait = t.Stop();
    if (DevSpecStatus < 0) { const int rc = DevSpecStatus; DevSpecStatus = 0; return Fail(rc, "sub-maps ahead of time (look-ahead thread)"); }
    Stats.maps_async = std::max(MapJobSeconds[0], std::max(MapJobSeconds[1], MapJobSeconds[2]));
    for (int k = 0; k < 3; ++k)
      if (MapJobFailed[k]) { MapJobFailed[k] = 0; return Fail(LSA_E_HIP, "lsa_device_grid_add_staged (map worker)"); }
    bool need[3], checking[3] = {false, false, false}, any = false;
    for (int k = 0; k < 3; ++k)
    {
      need[k] = UseKeypoints[k] && !lsa_device_grid_submap_valid(DevMaps[k]);
      any = any || need[k];
    }
    // the boxes of the current keypoints under the pose guess stay on the device: the grids read them there
    if (any && MapUpdate != MappingMode::NONE && !boxesEnqueued) LSA_TRY(lsa_keypoint_bboxes_begin(Ctx, LSA_SET_WORKING, Tworld.m));
    for (int k = 0; k < 3; ++k)
    {
      if (!need[k]) continue;
      lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, static_cast<float>((k == LSA_EDGE ? KnnCellScaleMapsEdges : KnnCellScaleMaps) * LocalMaps[k]->GetLeafSize()));
      if (MapUpdate == MappingMode::NONE) LSA_TRY(lsa_device_grid_build_submap_begin(DevMaps[k], nullptr, nullptr, -1, LSA_TARGET_MAP, k));
      else
      {
        // extracted ahead of time for the predicted box: stands when the actual box touches the same outer voxels (the
        // comparisons of all the maps are enqueued first, then waited for)
        if (DevSpec[k] && lsa_device_grid_submap_ahead_take_begin(DevMaps[k], k, KeypointCounts[k] / 2, LSA_TARGET_MAP, k) == 1) { checking[k] = true; continue; }
        if (LocalMaps[k]->IsTimeThreshold()) LSA_TRY(lsa_device_grid_clear_old_points(DevMaps[k], CurrentTime));
        LSA_TRY(lsa_device_grid_build_submap_begin_for_keypoints(DevMaps[k], k, KeypointCounts[k] / 2, LSA_TARGET_MAP, k));
      }
    }
    for (int k = 0; k < 3; ++k)
    {
      if (!checking[k]) continue;
      int taken = 0;
      LSA_TRY(lsa_device_grid_submap_ahead_take_end(DevMaps[k], &taken));
      if (taken) { need[k] = false; Stats.submap_spec_hits++; SubMapSpecHitsTotal++; continue; }
      if (LocalMaps[k]->IsTimeThreshold()) LSA_TRY(lsa_device_grid_clear_old_points(DevMaps[k], CurrentTime));
      LSA_TRY(lsa_device_grid_build_submap_begin_for_keypoints(DevMaps[k], k, KeypointCounts[k] / 2, LSA_TARGET_MAP, k));
    }
    for (bool& b : DevSpec) b = false;
    for (int k = 0; k < 3; ++k)  // the extractions follow one another on the context's stream, their sizes come back together
      if (need[k]) LSA_TRY(lsa_device_grid_build_submap_end(DevMaps[k]));
    Stats.submap += t.Stop();
    HoldLookahead = false;  // (the extraction is enqueued from the loop's interlude, behind this frame's first search: not here, in front of it)
  }
  else
  {
    Tick t;
    if (SpecPending)
    {
      const int rc = FinishSubMapSpeculation();
      if (rc < 0) return rc;
    }
    WaitMaps();  // the previous keyframe's insertion and the sub-maps extracted ahead of time
    Stats.maps_wait = t.Stop();
    Stats.maps_async = std::max(MapJobSeconds[0], std::max(MapJobSeconds[1], MapJobSeconds[2]));
    // which sub-maps are new (extracted ahead of time for the predicted pose) or stale (the map changed)
    bool fresh[3], rebuild[3] = {false, false, false};
    bool any = false;
    for (int k = 0; k < 3; ++k)
    {
      fresh[k] = UseKeypoints[k] && SpecBuilt[k];
      rebuild[k] = UseKeypoints[k] && !fresh[k] && !LocalMaps[k]->IsSubMapValid();
      any = any || fresh[k] || rebuild[k];
      SpecBuilt[k] = false;
    }
    float mn[9], mx[9];
    if (any && MapUpdate != MappingMode::NONE) LSA_TRY(lsa_working_bboxes(Ctx, Tworld.m, mn, mx));  // all types, one pass
    // A sub-map handed to the device ahead of time is only good for the prediction it was extracted for: whatever
    // does not hold gives it up here -- which also waits for the copy out of the staging buffer, so that the buffer
    // may be rewritten below.
    for (int k = 0; k < 3; ++k)
    {
      const bool holds = fresh[k] && MapUpdate != MappingMode::NONE && LocalMaps[k]->SubMapBuiltFor(mn + 3 * k, mx + 3 * k, KeypointCounts[k] / 2);
      if (SpecStaged[k] && !holds) LSA_TRY(lsa_drop_target_ahead(Ctx, LSA_TARGET_MAP, k));
      SpecStaged[k] = false;
      SpecDone[k].store(false);
    }
    for (int k = 0; k < 3; ++k)
    {
      if (!fresh[k] && !rebuild[k]) continue;
      RollingGrid* map = LocalMaps[k].get();
      const int minPts = KeypointCounts[k] / 2;
      if (fresh[k])
      {
        // the box under the actual pose touches the same voxels as the predicted one: the sub-map stands
        if (map->SubMapBuiltFor(mn + 3 * k, mx + 3 * k, minPts)) { Stats.submap_spec_hits++; SubMapSpecHitsTotal++; rebuild[k] = true; continue; }
        rebuild[k] = true;
      }

      if (MapUpdate == MappingMode::NONE)
        MapWorker[k].Submit([map] { map->BuildSubMap(); });
      else
      {
        const bool clear = map->IsTimeThreshold();
        const double now = CurrentTime;
        const float* lo3 = mn + 3 * k;
        const float* hi3 = mx + 3 * k;
        MapWorker[k].Submit([map, clear, now, minPts, mn0 = lo3[0], mn1 = lo3[1], mn2 = lo3[2], mx0 = hi3[0], mx1 = hi3[1], mx2 = hi3[2]] {
          if (clear) map->ClearOldPoints(now);
          const float lo[3] = {mn0, mn1, mn2}, hi[3] = {mx0, mx1, mx2};
          map->BuildSubMap(lo, hi, minPts);
        });
      }
    }
    for (int k = 0; k < 3; ++k)
    {
      if (!rebuild[k]) continue;
      MapWorker[k].Wait();
      // the map holds one point per leaf voxel: a search cell of about one leaf keeps a handful of candidates per cell
      lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, static_cast<float>((k == LSA_EDGE ? KnnCellScaleMapsEdges : KnnCellScaleMaps) * LocalMaps[k]->GetLeafSize()));
      // the worker extracted the sub-map straight into the target's pinned staging buffer: the copy is only enqueued
      LSA_TRY(lsa_set_target_staged(Ctx, LSA_TARGET_MAP, k, static_cast<int>(LocalMaps[k]->SubMapSize())));
    }
    Stats.submap += t.Stop();
  }

  const bool refined = Undistortion == UNDISTORTION_REFINED;
  IcpLoopSpec spec = {};
  spec.name = "loc";
  spec.target = LSA_TARGET_MAP;
  spec.set = LSA_SET_WORKING;
  for (int k = 0; k < 3; ++k)
    if (UseKeypoints[k]) spec.matchMask |= 1u << k;
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

int SlamCore::BeginSubMapSpeculation(const Pose& predicted)
{
  SpecPending = false;
  for (bool& b : DevSpec) b = false;
  if (MapUpdate == MappingMode::NONE) return LSA_OK;
  const bool onDevice = DeviceMapsInUse();
  if (onDevice)
  {
    // device maps: the sub-maps for the predicted boxes are extracted on the device, beside the ego-motion ICP; decaying
    // maps are left to the localization (ClearOldPoints comes first there)
    bool any = false;
    for (int k = 0; k < 3; ++k) any = any || (UseKeypoints[k] && KeypointCounts[k] > 0);
    if (!SubMapsAhead || !any || LocalMaps[0]->IsTimeThreshold()) return LSA_OK;
    // it has to be ready when the localization asks: where the ego-motion ICP is shorter than insertion + extraction +
    // grid build (small sensors) it is not, and is then left alone for a while
    if (DevSpecBackoff > 0) { --DevSpecBackoff; return LSA_OK; }
  }
  // Localization() will look at the keypoints after undistorting them with the motion between the previous pose
  // and the (then known) current one: the prediction does the same with the predicted pose -- the scan poses of
  // InterpolateScanPose at both ends of the keypoints' time range (Slam.cxx:1271-1285, 1288-1352).  Here Tworld
  // still is the previous frame's pose.
  bool interpolated = false;
  Pose begin = predicted, end = predicted;
  double t0 = 0., t1 = 0.;
  if (Undistortion && !LogTrajectory.empty())
  {
    LSA_TRY(lsa_keypoint_time_range(Ctx, LSA_SET_RAW_CURRENT, &t0, &t1));
    const double prevPoseTime = LogTrajectory.back().time;
    const double currPoseTime = StampToSec(CurrentStamp);
    if (t1 - t0 >= 1e-6 && currPoseTime != prevPoseTime)
    {
      auto scanPose = [&](double time) {
        if (std::abs(time / (currPoseTime - prevPoseTime)) > MaxExtrapolationRatio) return predicted;
        return LinearInterpolation(Tworld, predicted, currPoseTime + time, prevPoseTime, currPoseTime);
      };
      begin = scanPose(t0);
      end = scanPose(t1);
      interpolated = true;
    }
  }
  if (onDevice)
  {
    // Everything else is a dozen calls into the runtime: a host thread of its own
    // does it (the one that enqueues the next frame's ego-motion targets later in the frame), this one goes on to the
    // first search.  The boxes and the extractions go onto the grids' (look-ahead) stream, behind the previous keyframe's
    // insertions, the spare targets' search grids behind the extractions: nothing of it on the context's stream.
    int minPts[3];
    bool use[3];
    for (int k = 0; k < 3; ++k)
    {
      use[k] = UseKeypoints[k] && KeypointCounts[k] > 0;
      minPts[k] = KeypointCounts[k] / 2;
      if (use[k]) lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, static_cast<float>((k == LSA_EDGE ? KnnCellScaleMapsEdges : KnnCellScaleMaps) * LocalMaps[k]->GetLeafSize()));
      DevSpec[k] = use[k];
    }
    DevSpecStatus = 0;
    LSA_TRY(lsa_keypoint_boxes_predicted_mark(Ctx));  // the raw keypoints exist from here on the context's stream
    DevSpecRunning.store(true, std::memory_order_release);
    AheadWorker.Submit([this, interpolated, begin, end, t0, t1, use0 = use[0], use1 = use[1], use2 = use[2], m0 = minPts[0], m1 = minPts[1], m2 = minPts[2]] {
      const bool use[3] = {use0, use1, use2};
      const int minPts[3] = {m0, m1, m2};
      for (auto& w : MapWorker) w.Wait();  // the previous keyframe's insertions are on the grids' stream by now
      // the predicted boxes on the look-ahead stream, where the grids read them: nothing of this on the context's stream
      int rc = SpecBoxesOnLookahead ? lsa_keypoint_boxes_predicted(Ctx, LSA_SET_RAW_CURRENT, begin.m, interpolated ? end.m : nullptr, t0, t1)
                                    : (interpolated ? lsa_keypoint_bboxes_begin_interp(Ctx, LSA_SET_RAW_CURRENT, begin.m, end.m, t0, t1)
                                                    : lsa_keypoint_bboxes_begin(Ctx, LSA_SET_RAW_CURRENT, begin.m));
      for (int k = 0; k < 3 && rc >= 0; ++k)
        if (use[k]) rc = lsa_device_grid_submap_ahead_begin(DevMaps[k], k, minPts[k], k);
      // ... and waits for the extractions' sizes (this thread has nothing else to do) to enqueue the spare targets' search
      // grids at once.  The localization waits for this job to END (DevSpecRunning) before it touches the boxes' words or
      // the spare targets: nothing calls the job off half-way (the predicted boxes' kernels on the look-ahead stream have
      // to be over before lsa_keypoint_bboxes_begin rewrites those words on the context's stream)
      // (all the maps' grids in one sequence of launches, once the last size is there)
      lsa_device_grid* grids[3];
      int ng = 0;
      for (int k = 0; k < 3; ++k)
        if (use[k]) grids[ng++] = DevMaps[k];
      while (SpecGridsTogether && ng > 0 && rc >= 0)
      {
        rc = lsa_device_grid_submap_ahead_poll_all(grids, ng);
        if (rc != 1) break;
        std::this_thread::yield();
      }
      for (int i = 0; i < ng && !SpecGridsTogether && rc >= 0; ++i)
        while (rc >= 0)
        {
          rc = lsa_device_grid_submap_ahead_poll(grids[i]);
          if (rc != 1) break;
          std::this_thread::yield();
        }
      DevSpecStatus = rc < 0 ? rc : 0;
      DevSpecRunning.store(false, std::memory_order_release);
    });
    return LSA_OK;
  }
  if (interpolated) LSA_TRY(lsa_keypoint_bboxes_begin_interp(Ctx, LSA_SET_RAW_CURRENT, begin.m, end.m, t0, t1));
  else LSA_TRY(lsa_keypoint_bboxes_begin(Ctx, LSA_SET_RAW_CURRENT, predicted.m));
  SpecPending = true;
  return LSA_OK;
}

int SlamCore::FinishSubMapSpeculation()
{
  SpecPending = false;
  float mn[9], mx[9];
  LSA_TRY(lsa_keypoint_bboxes_end(Ctx, mn, mx));
  for (int k = 0; k < 3; ++k) { SpecDone[k].store(false); SpecStaged[k] = false; }
  for (int k = 0; k < 3; ++k)
  {
    if (!UseKeypoints[k] || KeypointCounts[k] <= 0) continue;
    RollingGrid* map = LocalMaps[k].get();
    const bool clear = map->IsTimeThreshold();
    const double now = CurrentTime;
    const int minPts = KeypointCounts[k] / 2;
    bool* built = &SpecBuilt[k];
    std::atomic<bool>* done = &SpecDone[k];
    const float* lo3 = mn + 3 * k;
    const float* hi3 = mx + 3 * k;
    // queued behind the previous keyframe's insertion on the same worker: it sees the final map
    MapWorker[k].Submit([map, clear, now, minPts, built, done, mn0 = lo3[0], mn1 = lo3[1], mn2 = lo3[2], mx0 = hi3[0], mx1 = hi3[1], mx2 = hi3[2]] {
      if (map->IsSubMapValid()) return;  // the map did not change: Slam.cxx:1013 keeps the kd-tree
      if (clear) map->ClearOldPoints(now);
      const float lo[3] = {mn0, mn1, mn2}, hi[3] = {mx0, mx1, mx2};
      map->BuildSubMap(lo, hi, minPts);
      *built = true;
      done->store(true, std::memory_order_release);
    });
  }
  return LSA_OK;
}

// Called between two steps of the ego-motion ICP: a sub-map the workers have finished for the predicted pose goes to
// the device right away -- upload and search grid on the look-ahead stream -- so that Localization(), if the
// prediction holds, only swaps it in.
int SlamCore::StageSpeculativeSubMaps()
{
  if (!BuildTargetsAhead) return LSA_OK;
  for (int k = 0; k < 3; ++k)
  {
    if (SpecStaged[k] || !SpecDone[k].load(std::memory_order_acquire)) continue;
    SpecStaged[k] = true;
    lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, static_cast<float>((k == LSA_EDGE ? KnnCellScaleMapsEdges : KnnCellScaleMaps) * LocalMaps[k]->GetLeafSize()));
    LSA_TRY(lsa_stage_target_ahead(Ctx, LSA_TARGET_MAP, k, static_cast<int>(LocalMaps[k]->SubMapSize())));
  }
  return LSA_OK;
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

// Slam::UpdateMapsUsingTworld (Slam.cxx:1178-1222)
int SlamCore::UpdateMapsUsingTworld()
{
  const Pose motion = Inverse(KfLastPose) * Tworld;
  const double trans = std::sqrt((motion(0, 3) * motion(0, 3) + motion(1, 3) * motion(1, 3)) + motion(2, 3) * motion(2, 3));
  const double rot = RotationAngle(motion);
  constexpr double MIN_KF_NB = 10.;
  WaitMaps();
  const double thresholdCoef = std::min(KfCounter / MIN_KF_NB, 1.);
  unsigned nbMapKpts = 0;
  const bool onDevice = DeviceMapsInUse();
  for (int k = 0; k < 3; ++k) nbMapKpts += onDevice ? static_cast<unsigned>(std::max(lsa_device_grid_size(DevMaps[k]), 0)) : LocalMaps[k]->Size();
  const bool isNewKeyFrame = nbMapKpts < MinNbMatchedKeypoints * 10 || trans >= thresholdCoef * KfDistanceThreshold ||
                             rot >= (thresholdCoef * KfAngleThreshold) / 180. * M_PI;
  if (!isNewKeyFrame) return LSA_OK;
  KfCounter++;
  KfLastPose = Tworld;
  for (double& v : MapJobSeconds) v = 0.;
  if (onDevice)
  {
    // the keyframe's keypoints go into the device maps as they are (WORLD transform, keying, sort, fold, merge: kernels on
    // the context's stream, nothing is waited for)
    // this thread only hands the keypoints over (one transform kernel per type); ONE worker enqueues the insertion of all
    // the types -- seven launches, a block row per map -- which runs on the look-ahead stream beside the next frame
    lsa_device_grid* grids[3];
    int types[3], ng = 0;
    for (int k = 0; k < 3; ++k)
    {
      if (!UseKeypoints[k]) continue;
      types[ng] = k;
      grids[ng++] = DevMaps[k];
    }
    if (ng > 0)
    {
      LSA_TRY(lsa_device_grid_stage_keypoints_all(grids, types, ng, LSA_SET_WORKING, Tworld.m));  // one transform launch for all the types
      const double time = CurrentTime;
      int* failed = &MapJobFailed[0];
      double* spent = &MapJobSeconds[0];
      MapWorker[0].Submit([g0 = grids[0], g1 = grids[1 % ng], g2 = grids[2 % ng], ng, time, failed, spent] {
        lsa_device_grid* gs[3] = {g0, g1, g2};
        Tick t;
        if (lsa_device_grid_add_staged_all(gs, ng, time) < 0) *failed = 1;
        *spent += t.Stop();  // host time of the enqueue (the kernels run on behind it)
      });
    }
    return LSA_OK;
  }
  // the device writes the world keypoints into pinned host memory; the map workers wait for exactly that and
  // insert them while this thread goes on with the next frame
  LSA_TRY(lsa_stage_transformed(Ctx, LSA_SET_WORKING, Tworld.m));
  for (int k = 0; k < 3; ++k)
  {
    if (!UseKeypoints[k]) continue;
    RollingGrid* map = LocalMaps[k].get();
    lsa_ctx* ctx = Ctx;
    const double time = CurrentTime;
    double* spent = &MapJobSeconds[k];
    MapWorker[k].Submit([map, ctx, k, time, spent] {
      map->WakeAddThreads();  // they are spinning by the time the staged keypoints have arrived
      const lsa_point_t* pts = nullptr;
      int n = 0;
      if (lsa_staged_transformed(ctx, k, &pts, &n) != LSA_OK) return;
      Tick t;
      map->Add(pts, static_cast<size_t>(std::max(n, 0)), false, time);
      *spent += t.Stop();
    });
  }
  return LSA_OK;
}

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

// Slam::GetMap / GetTargetSubMap (Slam.h:155-158)
int SlamCore::GetMap(int k, bool clean, std::vector<lsa_point_t>& out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (DeviceMapsInUse())
  {
    WaitMaps();
    const int size = std::max(lsa_device_grid_size(DevMaps[k]), 0);
    out.resize(size);
    const int n = size > 0 ? lsa_device_grid_get(DevMaps[k], clean ? 1 : 0, out.data(), size) : 0;
    if (n < 0) return Fail(n, "lsa_device_grid_get");
    out.resize(n);
    return n;
  }
  out = Map(k).Get(clean);
  return static_cast<int>(out.size());
}

void SlamCore::DropMapLookahead()
{
  SpecPending = false;
  for (int k = 0; k < 3; ++k)
  {
    SpecBuilt[k] = false;
    SpecDone[k].store(false);
    SpecStaged[k] = false;
    DevSpec[k] = false;
    if (Ctx) (void)lsa_drop_target_ahead(Ctx, LSA_TARGET_MAP, k);
  }
}

int SlamCore::AddMapPoints(int type, const lsa_point_t* pts, int n, bool fixed, double time)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (type < 0 || type > 2 || n < 0 || (n > 0 && !pts)) { LastError = "AddMapPoints: bad argument"; return LSA_E_ARG; }
  WaitMaps();
  DropMapLookahead();
  if (n == 0) return LSA_OK;
  if (DeviceMapsInUse()) LSA_TRY(lsa_device_grid_add(DevMaps[type], pts, n, fixed ? 1 : 0, time, 1));
  else LocalMaps[type]->Add(pts, static_cast<std::size_t>(n), fixed, time);
  return LSA_OK;
}

int SlamCore::SaveMapsToPCD(const std::string& prefix, int format, bool filtered, int counts[3])
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (format < pcd::kAscii || format > pcd::kBinaryCompressed) { LastError = "SaveMapsToPCD: unknown PCD format " + std::to_string(format); return LSA_E_ARG; }
  WaitMaps();
  for (int k = 0; k < 3; ++k)
  {
    if (counts) counts[k] = -1;
    if (!UseKeypoints[k]) continue;
    const std::string path = prefix + pcd::map_file_suffix(k);
    int n = 0;
    if (DeviceMapsInUse())
    {
      if (lsa_device_grid_size(DevMaps[k]) <= 0) continue;  // an empty cloud is not saved (PointCloudStorage.h:91-92)
      n = lsa_device_grid_save_pcd(DevMaps[k], path.c_str(), format, filtered ? 1 : 0);
      if (n < 0) return Fail(n, "lsa_device_grid_save_pcd");  // a file that cannot be written is an error, on either home of the maps
      if (n == 0) continue;  // (no voxel passed the filter)
    }
    else
    {
      const RollingGrid::PointCloud pts = LocalMaps[k]->Get(filtered);
      if (pts.empty()) continue;
      std::string err;
      const int rc = pcd::write_points(path, pts.data(), static_cast<long long>(pts.size()), format, err);
      if (rc < 0) { LastError = "SaveMapsToPCD: " + err; return LSA_E_ARG; }
      n = static_cast<int>(pts.size());
    }
    if (counts) counts[k] = n;
  }
  return LSA_OK;
}

int SlamCore::LoadMapsFromPCD(const std::string& prefix, bool resetMaps, double time, int counts[3])
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (resetMaps) ClearMaps();
  WaitMaps();
  DropMapLookahead();
  if (time < 0) time = static_cast<double>(std::time(nullptr));
  // "If mapping mode is NONE or ADD_DECAYING_KPTS, the first map points are fixed" (Slam.cxx:535-537)
  const bool fixedMap = MapUpdate == MappingMode::NONE || MapUpdate == MappingMode::ADD_KPTS_TO_FIXED_MAP;
  for (int k = 0; k < 3; ++k)
  {
    if (counts) counts[k] = -1;
    const std::string path = prefix + pcd::map_file_suffix(k);
    if (FILE* f = std::fopen(path.c_str(), "rb")) std::fclose(f);
    else continue;  // pcl::io::loadPCDFile(path) != 0: that map is left alone
    int n = 0;
    if (DeviceMapsInUse())
    {
      int format = 0;
      if (lsa_pcd_info(path.c_str(), &n, &format) != LSA_OK) { LastError = lsa_pcd_last_error(); return LSA_E_ARG; }
      LSA_TRY(lsa_device_grid_add_pcd(DevMaps[k], path.c_str(), fixedMap ? 1 : 0, time, 1));
    }
    else
    {
      std::vector<lsa_point_t> pts;
      std::string err;
      if (pcd::read_points(path, pts, err) != LSA_OK) { LastError = err; return LSA_E_ARG; }
      n = static_cast<int>(pts.size());
      if (n > 0) LocalMaps[k]->Add(pts.data(), pts.size(), fixedMap, time);
    }
    if (counts) counts[k] = n;
  }
  return LSA_OK;
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

// Slam::RunPoseGraphOptimization from "Update SLAM trajectory and maps" on (Slam.cxx:404-477); the optimizer is the caller's
int SlamCore::SetTrajectoryAndRebuildMaps(const double* poses17, int n)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const char* who = "SetTrajectoryAndRebuildMaps: ";
  if (LoggingTimeout == 0.) { LastError = std::string(who) + "keypoint logging is off (LoggingTimeout = 0): there is nothing to rebuild the maps from"; return LSA_E_STATE; }
  if (KpLogStopped) { LastError = std::string(who) + "keypoint logging stopped when a chunk could not be allocated; Reset(true) starts it again"; return LSA_E_STATE; }
  const int logged = static_cast<int>(LogTrajectory.size());
  if (!poses17 || n != logged) { LastError = std::string(who) + std::to_string(n) + " poses for " + std::to_string(logged) + " logged ones"; return LSA_E_ARG; }
  if (n < 2) { LastError = std::string(who) + "at least two poses"; return LSA_E_ARG; }
  for (int i = 0; i < n; ++i)
    if (!(poses17[17 * i + 16] == LogTrajectory[i].time))
    {
      LastError = std::string(who) + "pose " + std::to_string(i) + " is not dated like the logged one";
      return LSA_E_ARG;
    }
  if (lsa_kplog_size(Ctx) != n) { LastError = std::string(who) + "the keypoint log does not cover the logged poses (logging was switched on after the first of them)"; return LSA_E_STATE; }
  // (one Add per type, of any size the replay addresses: a long log takes the form of the device maps' insertion that keeps its
  //  scans in global memory, lsa_grid_add.hip)
  std::vector<double> poses(static_cast<size_t>(n) * 16), times(n);
  for (int i = 0; i < n; ++i)
  {
    std::memcpy(&poses[16 * static_cast<size_t>(i)], poses17 + 17 * static_cast<size_t>(i), 16 * sizeof(double));
    times[i] = poses17[17 * static_cast<size_t>(i) + 16];
  }
  // the map workers and the look-ahead are waited for, then what Reset(false) does (Slam.cxx:408)
  Reset(false);
  for (int i = 0; i < n; ++i) std::memcpy(LogTrajectory[i].pose.m, &poses[16 * static_cast<size_t>(i)], 16 * sizeof(double));
  unsigned mask = 0;
  for (int k = 0; k < 3; ++k)
    if (UseKeypoints[k]) mask |= 1u << k;
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
  return LSA_OK;
}

// ---- place recognition: which logged frame looks like this one (descriptors of the keypoint log, lsa_place.hip) -------------
int SlamCore::RecognizePlace(int query, const lsa_place_search_t* search, lsa_place_candidate_t* out, int capacity)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "RecognizePlace: ";
  if (capacity < 0 || (capacity > 0 && !out)) { LastError = who + "no place for the candidates"; return LSA_E_ARG; }
  if (LoggingTimeout == 0.) { LastError = who + "keypoint logging is off (LoggingTimeout = 0): there are no logged keypoints to describe"; return LSA_E_STATE; }
  if (KpLogStopped) { LastError = who + "keypoint logging stopped when a chunk could not be allocated; Reset(true) starts it again"; return LSA_E_STATE; }
  const int n = static_cast<int>(LogTrajectory.size());
  if (lsa_kplog_size(Ctx) != n) { LastError = who + "the keypoint log does not cover the logged poses (logging was switched on after the first of them)"; return LSA_E_STATE; }
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
  std::vector<double> rows(static_cast<size_t>(n) * 17);
  for (int i = 0; i < n; ++i)
  {
    std::memcpy(&rows[17 * static_cast<size_t>(i)], LogTrajectory[i].pose.m, 16 * sizeof(double));
    rows[17 * static_cast<size_t>(i) + 16] = LogTrajectory[i].time;
  }
  const int found = PlaceSelect(distance.data(), shift.data(), rows.data(), n, query, p.descriptor.sectors, p.min_travelled, p.max_distance, p.max_descriptor_distance,
                                p.exclusion_half_window, out, capacity);
  if (found < 0) LastError = who + "bad argument";
  return found;
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

int SlamCore::OptimizeLoggedTrajectory(const lsa_pgo_edge_t* loopEdges, int m, const lsa_pgo_params_t* params, double* poses17, int capacity, lsa_pgo_result_t* result)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "OptimizeLoggedTrajectory: ";
  if (!result || !poses17 || m < 0 || (m > 0 && !loopEdges)) { LastError = who + "bad argument"; return LSA_E_ARG; }
  if (LoggingTimeout == 0.) { LastError = who + "keypoint logging is off (LoggingTimeout = 0): there is no logged trajectory to optimize"; return LSA_E_STATE; }
  if (KpLogStopped) { LastError = who + "keypoint logging stopped when a chunk could not be allocated; Reset(true) starts it again"; return LSA_E_STATE; }
  const int n = static_cast<int>(LogTrajectory.size());
  if (lsa_kplog_size(Ctx) != n) { LastError = who + "the keypoint log does not cover the logged poses (logging was switched on after the first of them)"; return LSA_E_STATE; }
  lsa_pgo_params_t p;
  lsa_pgo_params_init(&p);
  if (params) p = *params;
  if (!pg::params_ok(p)) { LastError = who + "parameters out of limits"; return LSA_E_ARG; }
  if (n < 2) { LastError = who + "at least two logged poses"; return LSA_E_ARG; }
  if (capacity < n) { LastError = who + "room for " + std::to_string(capacity) + " of " + std::to_string(n) + " poses"; return LSA_E_ARG; }
  for (int k = 0; k < m; ++k)
    if (loopEdges[k].from < 0 || loopEdges[k].from >= n || loopEdges[k].to < 0 || loopEdges[k].to >= n || loopEdges[k].from == loopEdges[k].to)
    {
      LastError = who + "loop edge " + std::to_string(k) + " does not join two of the " + std::to_string(n) + " logged poses";
      return LSA_E_ARG;
    }
  std::vector<lsa_pgo_edge_t> edges(static_cast<size_t>(n - 1 + m));
  if (const int rc = LoggedChainEdges(p, who, edges.data()); rc != LSA_OK) return rc;
  for (int k = 0; k < m; ++k) edges[static_cast<size_t>(n - 1 + k)] = loopEdges[k];
  std::vector<double> in(static_cast<size_t>(n) * 16), out(static_cast<size_t>(n) * 16);
  std::vector<unsigned char> fixed(static_cast<size_t>(n), 0);
  fixed[0] = 1;
  for (int i = 0; i < n; ++i) std::memcpy(&in[16 * static_cast<size_t>(i)], LogTrajectory[i].pose.m, 16 * sizeof(double));
  {
    std::string why;
    if (const int rc = PgoCheckEdges(in.data(), n, edges.data(), static_cast<int>(edges.size()), &why); rc != LSA_OK) { LastError = who + why; return rc; }
  }
  // from here on the device works: the map workers and the look-ahead have enqueued what they had (nothing of theirs is changed)
  WaitMaps();
  if (const int rc = EnsureLoopClosureScratch(); rc < 0) return rc;
  (void)lsa_collect_garbage(LoopCtx);
  Tick t;
  lsa_pgo_result_t r;
  if (const int rc = lsa_pgo_solve(LoopCtx, in.data(), n, fixed.data(), edges.data(), static_cast<int>(edges.size()), &p, out.data(), &r); rc < 0)
  {
    LastError = who + lsa_last_error(LoopCtx);
    return rc;
  }
  PoseGraphSeconds = t.Stop();
  std::vector<double> rows(static_cast<size_t>(n) * 17);
  for (int i = 0; i < n; ++i)
  {
    std::memcpy(&rows[17 * static_cast<size_t>(i)], &out[16 * static_cast<size_t>(i)], 16 * sizeof(double));
    rows[17 * static_cast<size_t>(i) + 16] = LogTrajectory[i].time;
  }
  if (p.apply != 0)
    if (const int rc = SetTrajectoryAndRebuildMaps(rows.data(), n); rc < 0) return rc;
  std::memcpy(poses17, rows.data(), rows.size() * sizeof(double));
  *result = r;
  return n;
}

// ---- Slam::RunPoseGraphOptimization (Slam.cxx:355-477, PoseGraphOptimization::Process): GPS positions as priors -------------
int SlamCore::RunPoseGraphOptimization(const double* gpsTimes, const double* gpsXyz, const double* gpsCov9, int G, double* gpsToSensor16, double timeOffset,
                                       const lsa_pgo_params_t* params, double* poses17, int capacity, lsa_pgo_result_t* result)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "RunPoseGraphOptimization: ";
  if (!result || !poses17 || !gpsToSensor16 || G < 0 || (G > 0 && (!gpsTimes || !gpsXyz || !gpsCov9)) || !pg::finite_d(timeOffset)) { LastError = who + "bad argument"; return LSA_E_ARG; }
  if (LoggingTimeout == 0.) { LastError = who + "keypoint logging is off (LoggingTimeout = 0): there is no logged trajectory to optimize"; return LSA_E_STATE; }
  if (KpLogStopped) { LastError = who + "keypoint logging stopped when a chunk could not be allocated; Reset(true) starts it again"; return LSA_E_STATE; }
  const int n = static_cast<int>(LogTrajectory.size());
  if (lsa_kplog_size(Ctx) != n) { LastError = who + "the keypoint log does not cover the logged poses (logging was switched on after the first of them)"; return LSA_E_STATE; }
  lsa_pgo_params_t p;
  lsa_pgo_params_init(&p);
  if (params) p = *params;
  if (!pg::params_ok(p)) { LastError = who + "parameters out of limits"; return LSA_E_ARG; }
  if (n < 2 || G < 2)
  {
    LastError = who + "the SLAM and GPS trajectories must have at least 2 points (got " + std::to_string(n) + " logged poses and " + std::to_string(G) + " GPS positions)";
    return LSA_E_ARG;
  }
  if (capacity < n) { LastError = who + "room for " + std::to_string(capacity) + " of " + std::to_string(n) + " poses"; return LSA_E_ARG; }
  for (int k = 0; k < 16; ++k)
    if (!pg::finite_d(gpsToSensor16[k])) { LastError = who + "the GPS to sensor calibration has a non-finite entry"; return LSA_E_ARG; }
  for (int f = 0; f < G; ++f)
    for (int k = 0; k < 3; ++k)
      if (!pg::finite_d(gpsXyz[3 * static_cast<size_t>(f) + k]) || !pg::finite_d(gpsTimes[f])) { LastError = who + "GPS fix " + std::to_string(f) + " has a non-finite entry"; return LSA_E_ARG; }
  // the two tracks must overlap in time (PoseGraphOptimization.cxx:130-143; the logged times carry the offset here, and the
  // intervals are closed: the reference's strict comparison refuses two tracks that begin at the same instant, an accident)
  std::vector<double> times(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) times[static_cast<size_t>(i)] = LogTrajectory[i].time;
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
  std::vector<lsa_pgo_edge_t> edges(static_cast<size_t>(n - 1));
  if (const int rc = LoggedChainEdges(p, who, edges.data()); rc != LSA_OK) return rc;
  std::vector<double> in(static_cast<size_t>(n) * 16), start(in.size()), opt(in.size()), out(in.size());
  std::vector<unsigned char> fixed(static_cast<size_t>(n), 0);
  for (int i = 0; i < n; ++i) std::memcpy(&in[16 * static_cast<size_t>(i)], LogTrajectory[i].pose.m, 16 * sizeof(double));
  {
    std::string why;
    if (const int rc = PgoCheckEdges(in.data(), n, edges.data(), n - 1, &why); rc != LSA_OK) { LastError = who + why; return rc; }
  }
  // from here on the device works: the map workers and the look-ahead have enqueued what they had (nothing of theirs is changed)
  WaitMaps();
  if (const int rc = EnsureLoopClosureScratch(); rc < 0) return rc;
  (void)lsa_collect_garbage(LoopCtx);
  Tick t;
  lsa_pgo_result_t r;
  int rc = lsa_pgo_premultiply(LoopCtx, in.data(), n, W, start.data());
  if (rc == LSA_OK) rc = lsa_pgo_solve_priors(LoopCtx, start.data(), n, fixed.data(), edges.data(), n - 1, priors.data(), static_cast<int>(priors.size()), offset.m, &p, opt.data(), &r);
  if (rc == LSA_OK) rc = lsa_pgo_reanchor(LoopCtx, opt.data(), n, out.data());
  if (rc < 0)
  {
    LastError = who + lsa_last_error(LoopCtx);
    return rc;
  }
  PoseGraphSeconds = t.Stop();
  std::vector<double> rows(static_cast<size_t>(n) * 17);
  for (int i = 0; i < n; ++i)
  {
    std::memcpy(&rows[17 * static_cast<size_t>(i)], &out[16 * static_cast<size_t>(i)], 16 * sizeof(double));
    rows[17 * static_cast<size_t>(i) + 16] = LogTrajectory[i].time;
  }
  if (p.apply != 0)
    if (const int rc2 = SetTrajectoryAndRebuildMaps(rows.data(), n); rc2 < 0) return rc2;
  std::memcpy(poses17, rows.data(), rows.size() * sizeof(double));
  std::memcpy(gpsToSensor16, opt.data(), 16 * sizeof(double));  // the optimized pose 0 in the GPS frame (Slam.cxx:404)
  *result = r;
  return n;
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
  if (LoggingTimeout == 0.) { LastError = who + "keypoint logging is off (LoggingTimeout = 0): there are no logged keypoints to register against"; return LSA_E_STATE; }
  if (KpLogStopped) { LastError = who + "keypoint logging stopped when a chunk could not be allocated; Reset(true) starts it again"; return LSA_E_STATE; }
  const int n = static_cast<int>(LogTrajectory.size());
  if (lsa_kplog_size(Ctx) != n) { LastError = who + "the keypoint log does not cover the logged poses (logging was switched on after the first of them)"; return LSA_E_STATE; }
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

  unsigned mask = 0;
  for (int k = 0; k < 3; ++k)
    if (UseKeypoints[k]) mask |= 1u << k;
  const int rule = Undistortion != UNDISTORTION_NONE ? 2 : 0;
  std::vector<double> poses(static_cast<size_t>(n) * 16), times(n);
  for (int i = 0; i < n; ++i)
  {
    std::memcpy(&poses[16 * static_cast<size_t>(i)], LogTrajectory[i].pose.m, 16 * sizeof(double));
    times[i] = LogTrajectory[i].time;
  }
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
    lsa_set_target_cell_size(LoopCtx, LSA_TARGET_MAP, k, static_cast<float>((k == LSA_EDGE ? KnnCellScaleMapsEdges : KnnCellScaleMaps) * LocalMaps[k]->GetLeafSize()));
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
  lsa_set_fused_match(LoopCtx, FusedMatch ? 1 : 0);
  lsa_set_knn_lanes(LoopCtx, LSA_EDGE, KnnLanesEdges);
  lsa_set_knn_lanes(LoopCtx, LSA_PLANE, KnnLanesPlanes);
  lsa_set_knn_lanes(LoopCtx, LSA_BLOB, KnnLanesBlobs);
  lsa_set_knn_rounds(LoopCtx, LSA_EDGE, KnnRoundsEdges);
  lsa_set_knn_rounds(LoopCtx, LSA_PLANE, KnnRoundsPlanes);
  lsa_set_knn_rounds(LoopCtx, LSA_BLOB, KnnRoundsBlobs);
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

int SlamCore::GetTargetSubMap(int k, std::vector<lsa_point_t>& out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (DeviceMapsInUse())
  {
    const int size = std::max(lsa_target_size(Ctx, LSA_TARGET_MAP, k), 0);
    out.resize(size);
    if (size > 0) LSA_TRY(lsa_download_target(Ctx, LSA_TARGET_MAP, k, out.data(), size));
    return size;
  }
  const RollingGrid& map = Map(k);
  out.assign(map.SubMapData(), map.SubMapData() + map.SubMapSize());
  return static_cast<int>(out.size());
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

// name -> member table shared by SetParam / GetParam
#define LSA_PARAMS(X)                                                                                   \
  X("UseBlobs", UseKeypoints[LSA_BLOB], bool)                                                          \
  X("UseEdges", UseKeypoints[LSA_EDGE], bool)                                                          \
  X("UsePlanes", UseKeypoints[LSA_PLANE], bool)                                                        \
  X("TwoDMode", TwoDMode, bool)                                                                        \
  X("BuildTargetsAhead", BuildTargetsAhead, bool)                                                      \
  X("DeviceLM", DeviceLM, bool)                                                                        \
  X("MapsOnDevice", MapsOnDevice, bool)                                                                \
  X("SubMapsAhead", SubMapsAhead, bool)                                                                \
  X("SubMapsAheadAdaptive", SubMapsAheadAdaptive, bool)                                                \
  X("LocalizationStartFused", LocalizationStartFused, bool)                                            \
  X("WorkerPrewake", WorkerPrewake, bool)                                                              \
  X("ICPAhead", ICPAhead, int)                                                                         \
  X("UndistortInSearch", UndistortInSearch, bool)                                                      \
  X("SpecBoxesOnLookahead", SpecBoxesOnLookahead, bool)                                                \
  X("SpecGridsTogether", SpecGridsTogether, bool)                                                      \
  X("FusedMatch", FusedMatch, bool)                                                                    \
  X("EgoMotionICPMaxIter", EgoMotionICPMaxIter, unsigned)                                              \
  X("LocalizationICPMaxIter", LocalizationICPMaxIter, unsigned)                                        \
  X("EgoMotionLMMaxIter", EgoMotionLMMaxIter, unsigned)                                                \
  X("LocalizationLMMaxIter", LocalizationLMMaxIter, unsigned)                                          \
  X("EgoMotionMaxNeighborsDistance", EgoMotionMaxNeighborsDistance, double)                            \
  X("LocalizationMaxNeighborsDistance", LocalizationMaxNeighborsDistance, double)                      \
  X("EgoMotionEdgeNbNeighbors", EgoMotionEdgeNbNeighbors, unsigned)                                    \
  X("EgoMotionEdgeMinNbNeighbors", EgoMotionEdgeMinNbNeighbors, unsigned)                              \
  X("EgoMotionEdgeMaxModelError", EgoMotionEdgeMaxModelError, double)                                  \
  X("EgoMotionPlaneNbNeighbors", EgoMotionPlaneNbNeighbors, unsigned)                                  \
  X("EgoMotionPlanarityThreshold", EgoMotionPlanarityThreshold, double)                                \
  X("EgoMotionPlaneMaxModelError", EgoMotionPlaneMaxModelError, double)                                \
  X("EgoMotionInitSaturationDistance", EgoMotionInitSaturationDistance, double)                        \
  X("EgoMotionFinalSaturationDistance", EgoMotionFinalSaturationDistance, double)                      \
  X("LocalizationEdgeNbNeighbors", LocalizationEdgeNbNeighbors, unsigned)                              \
  X("LocalizationEdgeMinNbNeighbors", LocalizationEdgeMinNbNeighbors, unsigned)                        \
  X("LocalizationEdgeMaxModelError", LocalizationEdgeMaxModelError, double)                            \
  X("LocalizationPlaneNbNeighbors", LocalizationPlaneNbNeighbors, unsigned)                            \
  X("LocalizationPlanarityThreshold", LocalizationPlanarityThreshold, double)                          \
  X("LocalizationPlaneMaxModelError", LocalizationPlaneMaxModelError, double)                          \
  X("LocalizationBlobNbNeighbors", LocalizationBlobNbNeighbors, unsigned)                              \
  X("LocalizationInitSaturationDistance", LocalizationInitSaturationDistance, double)                  \
  X("LocalizationFinalSaturationDistance", LocalizationFinalSaturationDistance, double)                \
  X("MaxExtrapolationRatio", MaxExtrapolationRatio, double)                                            \
  X("MinNbMatchedKeypoints", MinNbMatchedKeypoints, unsigned)                                          \
  X("KfDistanceThreshold", KfDistanceThreshold, double)                                                \
  X("KfAngleThreshold", KfAngleThreshold, double)                                                      \
  X("KeepMatchDebug", KeepMatchDebug, bool)                                                            \
  X("KnnCellSizeEgoMotion", KnnCellSizeEgoMotion, double)                                              \
  X("KnnCellScaleMaps", KnnCellScaleMaps, double)                                                      \
  X("KnnCellSizeEgoMotionEdges", KnnCellSizeEgoMotionEdges, double)                                    \
  X("KnnCellScaleMapsEdges", KnnCellScaleMapsEdges, double)                                            \
  X("KnnLanesEdges", KnnLanesEdges, int)                                                               \
  X("KnnLanesPlanes", KnnLanesPlanes, int)                                                             \
  X("KnnLanesBlobs", KnnLanesBlobs, int)                                                               \
  X("KnnRoundsEdges", KnnRoundsEdges, int)                                                             \
  X("KnnRoundsPlanes", KnnRoundsPlanes, int)                                                           \
  X("KnnRoundsBlobs", KnnRoundsBlobs, int)                                                             \
  X("NeighborWidth", ExtractParams.neighbor_width, int)                                                \
  X("MinDistanceToSensor", ExtractParams.min_distance_to_sensor, float)                                \
  X("MinBeamSurfaceAngle", ExtractParams.min_beam_surface_angle, float)                                \
  X("PlaneSinAngleThreshold", ExtractParams.plane_sin_angle_threshold, float)                          \
  X("EdgeSinAngleThreshold", ExtractParams.edge_sin_angle_threshold, float)                            \
  X("DistToLineThreshold", ExtractParams.dist_to_line_threshold, float)                                \
  X("EdgeDepthGapThreshold", ExtractParams.edge_depth_gap_threshold, float)                            \
  X("EdgeSaliencyThreshold", ExtractParams.edge_saliency_threshold, float)                             \
  X("EdgeIntensityGapThreshold", ExtractParams.edge_intensity_gap_threshold, float)

// The maps live either in the device grids or in the host grids ("MapsOnDevice" = 0): a setter that
// moves them from one side to the other takes the points along, the way RollingGrid's own geometry setters do
// (prevMap = Get(); Clear(); Add(prevMap), RollingGrid.cxx:59-88: counts start again, the points keep their place).
int SlamCore::MigrateMaps(bool fromDevice)
{
  for (int k = 0; k < 3; ++k)
  {
    if (!DevMaps[k]) continue;
    if (fromDevice)
    {
      const int size = std::max(lsa_device_grid_size(DevMaps[k]), 0);
      std::vector<lsa_point_t> pts(static_cast<size_t>(size));
      const int n = size > 0 ? lsa_device_grid_get(DevMaps[k], 0, pts.data(), size) : 0;
      if (n < 0) return Fail(n, "lsa_device_grid_get");
      LocalMaps[k]->Clear();
      LocalMaps[k]->Add(pts.data(), static_cast<size_t>(n), false, CurrentTime);
      LSA_TRY(lsa_device_grid_clear(DevMaps[k]));
    }
    else
    {
      const RollingGrid::PointCloud pts = LocalMaps[k]->Get();
      LSA_TRY(lsa_device_grid_clear(DevMaps[k]));
      if (!pts.empty()) LSA_TRY(lsa_device_grid_add(DevMaps[k], pts.data(), static_cast<int>(pts.size()), 0, CurrentTime, 1));
      LocalMaps[k]->Clear();
    }
  }
  return LSA_OK;
}

int SlamCore::SetParam(const std::string& name, double v)
{
  WaitMaps();
  const bool onDevice = DeviceMapsInUse();
  const int rc = SetParamValue(name, v);
  if (rc == LSA_OK && DeviceMapsInUse() != onDevice) return MigrateMaps(onDevice);
  return rc;
}

int SlamCore::SetParamValue(const std::string& name, double v)
{
#define X(NAME, MEMBER, TYPE) if (name == NAME) { MEMBER = static_cast<TYPE>(v); return LSA_OK; }
  LSA_PARAMS(X)
#undef X
  if (name == "WheelOdomWeight") { SensorManagers.SetWheelOdomWeight(v); return LSA_OK; }
  if (name == "GravityWeight") { SensorManagers.SetGravityWeight(v); return LSA_OK; }
  if (name == "SensorTimeOffset") { SensorManagers.SetTimeOffset(v); return LSA_OK; }
  if (name == "NbThreads") return LSA_OK;  // OpenMP thread count of the reference: no meaning on the device path
  if (name == "Verbosity") return LSA_OK;
  if (name == "EgoMotion") { EgoMotion = static_cast<EgoMotionMode>(static_cast<int>(v)); return LSA_OK; }
  if (name == "Undistortion") { Undistortion = static_cast<UndistortionMode>(static_cast<int>(v)); return LSA_OK; }
  if (name == "MapUpdate") { MapUpdate = static_cast<MappingMode>(static_cast<int>(v)); return LSA_OK; }
  if (name == "OverlapSamplingRatio")
  {
    // Slam::SetOverlapSamplingRatio (Slam.cxx:1359-1367)
    OverlapSamplingRatio = std::min(std::max(static_cast<float>(v), 0.f), 1.f);
    if (OverlapSamplingRatio == 0.f) OverlapEstimation = -1.f;
    return LSA_OK;
  }
  if (name == "MapAddThreads") { LocalMaps[LSA_PLANE]->SetAddThreads(static_cast<int>(v)); return LSA_OK; }
  if (name == "MapAddThreadsEdges") { LocalMaps[LSA_EDGE]->SetAddThreads(static_cast<int>(v)); return LSA_OK; }
  if (name == "LoggingTimeout")
  {
    LoggingTimeout = v;
    // logging off: the poses are trimmed to two at the next frame, and keypoints logged so far would describe none of them
    if (v == 0. && Ctx) { (void)lsa_kplog_clear(Ctx); KpLogStopped = false; }
    return LSA_OK;
  }
  if (name == "LoggingStorage")
  {
    // PointCloudStorageType (PointCloudStorage.h:68-75): all five are accepted and mean the same here, uncompressed in HBM
    if (!(v >= 0 && v <= 4)) { LastError = "LoggingStorage: a PointCloudStorageType (0..4)"; return LSA_E_ARG; }
    LoggingStorage = static_cast<int>(v);
    return LSA_OK;
  }
  if (name == "TimeWindowDuration") { TimeWindowDuration = static_cast<float>(v); return LSA_OK; }
  if (name == "VelocityLimitLinear") { VelocityLimits[0] = static_cast<float>(v); return LSA_OK; }
  if (name == "VelocityLimitAngular") { VelocityLimits[1] = static_cast<float>(v); return LSA_OK; }
  if (name == "AccelerationLimitLinear") { AccelerationLimits[0] = static_cast<float>(v); return LSA_OK; }
  if (name == "AccelerationLimitAngular") { AccelerationLimits[1] = static_cast<float>(v); return LSA_OK; }
  if (name == "AzimuthalResolution") { if (Ctx) lsa_set_azimuthal_resolution(Ctx, static_cast<float>(v)); return LSA_OK; }
  auto dev = [&](int k, const char* what, double value) { if (DevMaps[k]) lsa_device_grid_set(DevMaps[k], what, value); };
  if (name == "VoxelGridLeafSizeEdges") { LocalMaps[LSA_EDGE]->SetLeafSize(v); dev(LSA_EDGE, "LeafSize", v); return LSA_OK; }
  if (name == "VoxelGridLeafSizePlanes") { LocalMaps[LSA_PLANE]->SetLeafSize(v); dev(LSA_PLANE, "LeafSize", v); return LSA_OK; }
  if (name == "VoxelGridLeafSizeBlobs") { LocalMaps[LSA_BLOB]->SetLeafSize(v); dev(LSA_BLOB, "LeafSize", v); return LSA_OK; }
  if (name == "VoxelGridSize") { for (int k = 0; k < 3; ++k) { LocalMaps[k]->SetGridSize(static_cast<int>(v)); dev(k, "GridSize", v); } return LSA_OK; }
  if (name == "VoxelGridResolution") { for (int k = 0; k < 3; ++k) { LocalMaps[k]->SetVoxelResolution(v); dev(k, "VoxelResolution", v); } return LSA_OK; }
  if (name == "VoxelGridMinFramesPerVoxel") { for (int k = 0; k < 3; ++k) { LocalMaps[k]->SetMinFramesPerVoxel(static_cast<unsigned>(v)); dev(k, "MinFramesPerVoxel", v); } return LSA_OK; }
  if (name == "VoxelGridDecayingThreshold") { for (int k = 0; k < 3; ++k) { LocalMaps[k]->SetDecayingThreshold(v); dev(k, "DecayingThreshold", v); } return LSA_OK; }
  if (name == "VoxelGridSamplingMode") { for (int k = 0; k < 3; ++k) { LocalMaps[k]->SetSampling(static_cast<SamplingMode>(static_cast<int>(v))); dev(k, "Sampling", v); } return LSA_OK; }
  if (name == "OrderedMaps")
  {
    // both homes of the maps: the host grids, and the device grids (which put the points they hold back in, in the order
    // they hand them out now, the way the geometry setters do: time -1, not fixed, so decaying device maps lose them at
    // the next ClearOldPoints -- set it before the first frame)
    OrderedMaps = v != 0;
    for (auto& m : LocalMaps) m->SetOrdered(OrderedMaps);
    for (int k = 0; k < 3; ++k)
      if (DevMaps[k] && lsa_device_grid_set(DevMaps[k], "Ordered", OrderedMaps ? 1. : 0.) != LSA_OK) return Fail(LSA_E_HIP, "lsa_device_grid_set(Ordered)");
    return LSA_OK;
  }
  LastError = "unknown parameter " + name;
  return LSA_E_ARG;
}

int SlamCore::GetParam(const std::string& name, double* v) const
{
  if (!v) return LSA_E_ARG;
#define X(NAME, MEMBER, TYPE) if (name == NAME) { *v = static_cast<double>(MEMBER); return LSA_OK; }
  LSA_PARAMS(X)
#undef X
  if (name == "EgoMotion") { *v = static_cast<int>(EgoMotion); return LSA_OK; }
  if (name == "Undistortion") { *v = static_cast<int>(Undistortion); return LSA_OK; }
  if (name == "MapUpdate") { *v = static_cast<int>(MapUpdate); return LSA_OK; }
  if (name == "WheelOdomWeight") { *v = SensorManagers.GetWheelOdomWeight(); return LSA_OK; }
  if (name == "GravityWeight") { *v = SensorManagers.GetGravityWeight(); return LSA_OK; }
  if (name == "SensorTimeOffset") { *v = SensorManagers.GetTimeOffset(); return LSA_OK; }
  if (name == "AzimuthalResolution") { *v = Ctx ? lsa_get_azimuthal_resolution(Ctx) : 0.; return LSA_OK; }
  if (name == "VoxelGridLeafSizeEdges") { *v = LocalMaps[LSA_EDGE]->GetLeafSize(); return LSA_OK; }
  if (name == "VoxelGridLeafSizePlanes") { *v = LocalMaps[LSA_PLANE]->GetLeafSize(); return LSA_OK; }
  if (name == "VoxelGridLeafSizeBlobs") { *v = LocalMaps[LSA_BLOB]->GetLeafSize(); return LSA_OK; }
  if (name == "VoxelGridSize") { *v = LocalMaps[0]->GetGridSize(); return LSA_OK; }
  if (name == "VoxelGridResolution") { *v = LocalMaps[0]->GetVoxelResolution(); return LSA_OK; }
  if (name == "VoxelGridSamplingMode") { *v = static_cast<int>(LocalMaps[0]->GetSampling()); return LSA_OK; }
  if (name == "VoxelGridDecayingThreshold") { *v = LocalMaps[0]->GetDecayingThreshold(); return LSA_OK; }
  if (name == "VoxelGridMinFramesPerVoxel") { *v = LocalMaps[0]->GetMinFramesPerVoxel(); return LSA_OK; }
  if (name == "NbrFrameProcessed") { *v = NbrFrameProcessed; return LSA_OK; }
  if (name == "TotalMatchedKeypoints") { *v = TotalMatchedKeypoints; return LSA_OK; }
  if (name == "OverlapSamplingRatio") { *v = OverlapSamplingRatio; return LSA_OK; }
  if (name == "OverlapEstimation") { *v = OverlapEstimation; return LSA_OK; }
  if (name == "SubMapSpeculationHits") { *v = SubMapSpecHitsTotal; return LSA_OK; }
  if (name == "LookaheadAdopted") { *v = Ctx ? lsa_extract_prefetch_adopted(Ctx) : 0; return LSA_OK; }
  if (name == "OrderedMaps") { *v = OrderedMaps ? 1. : 0.; return LSA_OK; }
  if (name == "DeviceMapsInUse") { *v = DeviceMapsInUse() ? 1. : 0.; return LSA_OK; }
  if (name == "UploadsAdopted") { *v = Ctx ? lsa_uploads_adopted(Ctx) : 0; return LSA_OK; }
  if (name == "DeviceSolveFallbacks") { *v = Ctx ? lsa_solve_device_fallbacks(Ctx) : 0; return LSA_OK; }
  if (name == "IcpGateTimeouts") { *v = 0; return LSA_OK; }  // nothing counts them any more: the benchmark still reads the name
  if (name == "TargetsBuiltAheadAdopted") { *v = Ctx ? lsa_prepared_targets_adopted(Ctx) : 0; return LSA_OK; }
  if (name == "SubMapsStagedAheadAdopted") { *v = Ctx ? lsa_staged_targets_adopted(Ctx) : 0; return LSA_OK; }
  if (name == "MapAddThreads") { *v = LocalMaps[LSA_PLANE]->GetAddThreads(); return LSA_OK; }
  if (name == "MapAddThreadsEdges") { *v = LocalMaps[LSA_EDGE]->GetAddThreads(); return LSA_OK; }
  if (name == "LoggingTimeout") { *v = LoggingTimeout; return LSA_OK; }
  if (name == "LoggingStorage") { *v = LoggingStorage; return LSA_OK; }
  // the last RegisterLoggedFrames by the host's clock (every stage ends in a wait for the device): the two replays, the
  // scratch maps' insertions and sub-maps, the ICP loop with the registration error, the whole call
  if (name == "LoopClosureReplaySeconds") { *v = LoopClosureSeconds[0]; return LSA_OK; }
  if (name == "LoopClosureMapsSeconds") { *v = LoopClosureSeconds[1]; return LSA_OK; }
  if (name == "LoopClosureIcpSeconds") { *v = LoopClosureSeconds[2]; return LSA_OK; }
  if (name == "LoopClosureSeconds") { *v = LoopClosureSeconds[3]; return LSA_OK; }
  if (name == "PoseGraphSeconds") { *v = PoseGraphSeconds; return LSA_OK; }
  if (name == "LoggedKeypointsBytes") { *v = Ctx ? static_cast<double>(lsa_kplog_bytes(Ctx)) : 0.; return LSA_OK; }
  if (name == "LoggedFrames") { *v = LoggedFrames(); return LSA_OK; }
  if (name == "TimeWindowDuration") { *v = TimeWindowDuration; return LSA_OK; }
  if (name == "VelocityLimitLinear") { *v = VelocityLimits[0]; return LSA_OK; }
  if (name == "VelocityLimitAngular") { *v = VelocityLimits[1]; return LSA_OK; }
  if (name == "AccelerationLimitLinear") { *v = AccelerationLimits[0]; return LSA_OK; }
  if (name == "AccelerationLimitAngular") { *v = AccelerationLimits[1]; return LSA_OK; }
  if (name == "ComplyMotionLimits") { *v = ComplyMotionLimits ? 1. : 0.; return LSA_OK; }
  if (name == "Latency") { *v = Latency; return LSA_OK; }
  return LSA_E_ARG;
}

}  // namespace host
}  // namespace lsa
