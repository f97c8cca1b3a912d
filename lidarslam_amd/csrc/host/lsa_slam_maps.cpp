// lsa_slam_maps.cpp -- SlamCore's maps: the sub-maps a localization searches (which are stale, what the speculation left,
// the extractions), the sub-maps extracted ahead of time, the keyframe's insertion, reading, loading and saving.
#include "lsa_slam_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include "lsa_pcd.h"
#include "lsa_place.h"

namespace lsa
{
namespace host
{
// The part of Slam::Localization between its first undistortion and its ICP loop (Slam.cxx:1003-1037): the sub-maps of the
// maps whose last keyframe changed them, under the box of the working keypoints at the pose guess Tworld.  What the
// speculation extracted for the predicted box is taken where it stands and dropped where not.  boxesEnqueued: the boxes
// are on the device already (lsa_localization_begin).  Two homes of the maps, two different procedures.
int SlamCore::PrepareLocalizationSubMaps(bool boxesEnqueued)
{
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
      lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, MapSearchCell(k));
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
      lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, MapSearchCell(k));
      // the worker extracted the sub-map straight into the target's pinned staging buffer: the copy is only enqueued
      LSA_TRY(lsa_set_target_staged(Ctx, LSA_TARGET_MAP, k, static_cast<int>(LocalMaps[k]->SubMapSize())));
    }
    Stats.submap += t.Stop();
  }
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
      if (use[k]) lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, MapSearchCell(k));
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
    lsa_set_target_cell_size(Ctx, LSA_TARGET_MAP, k, MapSearchCell(k));
    LSA_TRY(lsa_stage_target_ahead(Ctx, LSA_TARGET_MAP, k, static_cast<int>(LocalMaps[k]->SubMapSize())));
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

// ---- place recognition against the maps: where in a loaded map is the vehicle (lsa_map_place.hip) -----------
int SlamCore::RecognizePlaceInMaps(const double* viewpoints, int V, const lsa_map_place_search_t* search, lsa_map_place_candidate_t* out, int capacity,
                                   lsa_map_place_summary_t* summary)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  const std::string who = "RecognizePlaceInMaps: ";
  if (capacity < 0 || (capacity > 0 && !out)) { LastError = who + "no place for the candidates"; return LSA_E_ARG; }
  lsa_map_place_search_t p;
  lsa_map_place_search_init(&p);
  if (search) p = *search;
  if (!MapSearchOk(p)) { LastError = who + "parameters out of limits"; return LSA_E_ARG; }
  if (!viewpoints || V < 1) { LastError = who + "at least one viewpoint"; return LSA_E_ARG; }
  for (size_t i = 0; i < 3 * static_cast<size_t>(V); ++i)
    if (!(viewpoints[i] - viewpoints[i] == 0.)) { LastError = who + "viewpoint " + std::to_string(i / 3) + " is not finite"; return LSA_E_ARG; }
  const lsa_place_params_t& d = p.descriptor;
  lsa_map_place_summary_t sum;
  std::memset(&sum, 0, sizeof(sum));
  sum.viewpoints = V;
  long long queryPoints = 0;
  for (int k = 0; k < 3; ++k)
    if ((d.type_mask >> k) & 1u) queryPoints += sum.query_points[k] = std::max(lsa_keypoint_count(Ctx, LSA_SET_RAW_CURRENT, k), 0);
  if (queryPoints == 0)
  {
    LastError = who + "there are no keypoints to describe: no frame has been added since construction, Reset or SetWorldTransformFromGuess";
    return LSA_E_STATE;
  }
  // the device works from here on: the map workers and the look-ahead have enqueued what they had (nothing of theirs is changed)
  WaitMaps();
  const bool onDevice = DeviceMapsInUse();
  long long mapPoints = 0;
  for (int k = 0; k < 3; ++k)
    if ((d.type_mask >> k) & 1u)
      mapPoints += sum.map_points[k] = onDevice ? static_cast<long long>(lsa_device_grid_get_param(DevMaps[k], "Voxels")) : static_cast<long long>(LocalMaps[k]->Size());
  if (mapPoints == 0) { LastError = who + "every map of the type mask is empty"; return LSA_E_STATE; }
  int described = 0;
  if (onDevice)
  {
    MapPlaceHostTable.valid = false;
    lsa_device_grid* grids[3] = {DevMaps[0], DevMaps[1], DevMaps[2]};
    described = lsa_map_place_describe_grids(Ctx, grids, &d, viewpoints, V);
  }
  else
  {
    HostMapTable& t = MapPlaceHostTable;
    bool same = t.valid && std::memcmp(&t.params, &d, sizeof(d)) == 0 && t.viewpoints.size() == 3 * static_cast<size_t>(V) &&
                std::memcmp(t.viewpoints.data(), viewpoints, t.viewpoints.size() * sizeof(double)) == 0;
    for (int k = 0; k < 3 && same; ++k)
      if ((d.type_mask >> k) & 1u) same = t.modifications[k] == LocalMaps[k]->GetModifications();
    if (!same)
    {
      // Get into one array, which the context uploads and describes
      t.valid = false;
      std::vector<lsa_point_t> all;
      all.reserve(static_cast<size_t>(mapPoints));
      for (int k = 0; k < 3; ++k)
        if ((d.type_mask >> k) & 1u)
        {
          const RollingGrid::PointCloud pts = LocalMaps[k]->Get();
          all.insert(all.end(), pts.begin(), pts.end());
          t.modifications[k] = LocalMaps[k]->GetModifications();
        }
      described = lsa_map_place_describe_points(Ctx, &d, all.data(), static_cast<int>(all.size()), viewpoints, V);
      if (described >= 0)
      {
        t.params = d;
        t.viewpoints.assign(viewpoints, viewpoints + 3 * static_cast<size_t>(V));
        t.valid = true;
      }
    }
  }
  if (described < 0) { LastError = who + lsa_last_error(Ctx); return described; }
  sum.described = described;
  std::vector<float> distance(static_cast<size_t>(V));
  std::vector<int32_t> shift(static_cast<size_t>(V));
  if (const int rc = lsa_map_place_search(Ctx, &d, LSA_SET_RAW_CURRENT, distance.data(), shift.data()); rc < 0)
  {
    LastError = who + lsa_last_error(Ctx);
    return rc;
  }
  const int found = MapPlaceSelect(distance.data(), shift.data(), viewpoints, V, d.sectors, p, out, capacity);
  if (found < 0) { LastError = who + "bad argument"; return found; }
  if (summary) *summary = sum;
  return found;
}

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

}  // namespace host
}  // namespace lsa
