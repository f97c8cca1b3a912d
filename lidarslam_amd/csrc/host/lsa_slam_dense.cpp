// lsa_slam_dense.cpp -- see lsa_slam_core.h: the pipeline's dense point-cloud map (lsa_dense_*.hip).  The
// registered frame goes into the table at the end of AddFrame without leaving the device; what moves the poses under the
// points that are already in it clears it -- or, under "DenseMapOnTrajectory" 1 and for an applied trajectory alone,
// re-projects it: every voxel's point moved by the correction of the frame that measured it.  Under "DenseMapCarve" 1 the rays
// of the inserted frames are walked through the table behind the insertions (free space: misses per voxel, filter, prune).
#include "lsa_slam_internal.h"
#include <algorithm>
#include <cstdio>
#include <cstring>

namespace lsa
{
namespace host
{
// The frame or frames of the call under exactly the poses GetRegisteredFrame uses, fused with the insertion, on the
// look-ahead stream; nothing is waited for.  A refused insertion (the table would outgrow "DenseMapMaxBytes") is counted
// and reported, and does not fail the frame.
int SlamCore::MakeDenseMap()
{
  if (Dense) return LSA_OK;
  LSA_TRY(lsa_dense_map_create(Ctx, DenseMapLeafSize, &Dense));
  LSA_TRY(lsa_dense_map_set(Dense, "MaxBytes", DenseMapMaxBytes));
  LSA_TRY(lsa_dense_map_set(Dense, "GridMaxCells", DenseMapGridMaxCells));
  if (DenseMapCarve) LSA_TRY(SetDenseCarveParams());
  return LSA_OK;
}

int SlamCore::InsertDenseFrame(bool keyframe, double time)
{
  if (DenseMapMode == 2 && !keyframe) return LSA_OK;
  LSA_TRY(MakeDenseMap());
  const int ordinal = static_cast<int>(DenseFrames);
  bool inserted = false, refused = false;
  // the ordinal's viewpoint: where the sensor of the call's first frame stands under the pose of the insertion
  const Pose view = Tworld * (CurrentFrames.empty() ? BaseToLidarOffset : GetBaseToLidarOffset(CurrentFrames.front().device));
  // the frame in use under the poses GetRegisteredFrame uses: inserted, or (carve) its rays walked
  auto insert = [&](const Pose& offset, double timeOffset, bool carve = false) -> int {
    int rc;
    if (Undistortion)
    {
      const Pose H0 = (Tworld * Motion.GetH0()) * offset;
      const Pose H1 = (Tworld * Motion.GetH1()) * offset;
      rc = (carve ? lsa_dense_map_carve_frame : lsa_dense_map_insert_frame)(Dense, 1, H0.m, H1.m, Motion.Time0, Motion.Time1, timeOffset, ordinal);
    }
    else
    {
      const Pose tf = Tworld * offset;
      rc = (carve ? lsa_dense_map_carve_frame : lsa_dense_map_insert_frame)(Dense, 0, tf.m, nullptr, 0., 0., timeOffset, ordinal);
    }
    if (carve) return rc < 0 ? Fail(rc, "lsa_dense_map_carve_frame") : LSA_OK;
    if (rc == LSA_E_CAPACITY)
    {
      refused = true;
      LastError = std::string("dense map: frame not inserted: ") + lsa_last_error(Ctx);
      return LSA_OK;
    }
    if (rc < 0) return Fail(rc, "lsa_dense_map_insert_frame");
    inserted = true;
    return LSA_OK;
  };
  if (!CurrentFrames.empty())
  {
    // the call is inserted whole or not at all: room for all its device frames is made before the first of them goes in
    long long total = 0;
    for (const HeldFrame& f : CurrentFrames) total += f.n;
    if (const int rc = lsa_dense_map_reserve(Dense, total); rc == LSA_E_CAPACITY)
    {
      DenseRefused++;
      LastError = std::string("dense map: frames not inserted: ") + lsa_last_error(Ctx);
      return LSA_OK;
    }
    else if (rc < 0) return Fail(rc, "lsa_dense_map_reserve");
    // AggregateFrames(CurrentFrames, true): every device frame with its own offset and time shift, one ordinal for the call
    for (const HeldFrame& f : CurrentFrames)
    {
      LSA_TRY(lsa_frame_store_use(Ctx, f.slot));
      if (const int rc = insert(GetBaseToLidarOffset(f.device), f.timeOffset); rc < 0) return rc;
    }
  }
  else if (lsa_frame_size(Ctx) > 0)
  {
    if (const int rc = insert(BaseToLidarOffset, 0.); rc < 0) return rc;
  }
  if (refused) DenseRefused++;
  if (DenseMapCarve && inserted && !refused)
  {
    // free space: only now that every device frame of the call is in the map -- a voxel the second LiDAR hit carries this
    // ordinal and is not seen through by the first
    if (!CurrentFrames.empty())
    {
      for (const HeldFrame& f : CurrentFrames)
      {
        LSA_TRY(lsa_frame_store_use(Ctx, f.slot));
        if (const int rc = insert(GetBaseToLidarOffset(f.device), f.timeOffset, true); rc < 0) return rc;
      }
    }
    else if (const int rc = insert(BaseToLidarOffset, 0., true); rc < 0) return rc;
  }
  if (inserted)
  {
    DenseLastOrdinal = ordinal;
    DenseFrames++;
    DenseTimes.push_back(time);  // 8 B a frame: which logged pose an applied trajectory corrects this ordinal by
    for (int a = 0; a < 3; ++a) DenseViewpoints.push_back(static_cast<float>(view.m[4 * a + 3]));  // 12 B a frame: what the normals are turned towards
  }
  return LSA_OK;
}

// Reset, ClearMaps, a corrected trajectory: the points in the map were placed under poses that no longer hold -- also while
// "DenseMap" is 0 for the moment: a map made before must not come back stale when it is switched on again
void SlamCore::DropDenseMap(const char* why)
{
  if (!Dense) return;
  (void)lsa_dense_map_clear(Dense);
  DenseFrames = 0;
  DenseLastOrdinal = -1;
  DenseTimes.clear();
  DenseViewpoints.clear();
  DenseClears++;
  if (why && !DenseWarned)
  {
    DenseWarned = true;
    std::fprintf(stderr, "lidarslam_amd: the dense map was cleared by %s: its points were placed under the poses of before, and raw frames are not logged to place them again (said once)\n", why);
  }
}

// SetTrajectoryAndRebuildMaps, before the logged poses are overwritten: D_i = new_i * inverse(old_i) per logged pose, then per
// dense ordinal the correction of the logged pose with its time.  Ordinals older than the log (a positive LoggingTimeout)
// precede *firstOrdinal and take the oldest logged pose's correction: the clamp of lsa_dense_map_reproject.
bool SlamCore::DenseCorrections(const double* poses16, int n, std::vector<double>& corrections, int* firstOrdinal) const
{
  if (DenseMapOnTrajectory != 1 || !Dense || DenseFrames == 0 || DenseTimes.size() != DenseFrames || n < 1) return false;
  std::vector<double> old, times, D(static_cast<size_t>(n) * 16);
  LoggedPoses16(old, &times);
  if (lsa_pose_corrections(old.data(), poses16, n, D.data()) != LSA_OK) return false;
  const size_t first = static_cast<size_t>(std::lower_bound(DenseTimes.begin(), DenseTimes.end(), times[0]) - DenseTimes.begin());
  corrections.clear();
  size_t i = 0;
  for (size_t j = first; j < DenseTimes.size(); ++j)
  {
    // the logged pose dated like the ordinal (the last one not after it, should a time ever be missing from the log)
    while (i + 1 < static_cast<size_t>(n) && times[i + 1] <= DenseTimes[j]) ++i;
    corrections.insert(corrections.end(), D.begin() + 16 * i, D.begin() + 16 * (i + 1));
  }
  if (corrections.empty()) corrections.assign(D.begin(), D.begin() + 16);  // every ordinal is older than the log
  *firstOrdinal = static_cast<int>(first);
  return true;
}

// The map under the corrections; the ordinals go on.  Without memory for the second table the map is cleared as under
// "DenseMapOnTrajectory" 0, counted in "DenseMapClears", the reason in LastError: the trajectory is applied all the same.
int SlamCore::ReprojectDenseMap(const std::vector<double>& corrections, int firstOrdinal)
{
  long long dropped = 0;
  const int rc = lsa_dense_map_reproject(Dense, corrections.data(), firstOrdinal, static_cast<int>(corrections.size() / 16), &dropped);
  if (rc == LSA_OK)
  {
    DenseReprojections++;
    // every viewpoint moves as the voxels of its ordinal moved: the clamp and the arithmetic of the re-projection (rigid_apply
    // in double, without contraction, narrowed to float)
    const long long n = static_cast<long long>(corrections.size() / 16);
    for (size_t j = 0; 3 * j + 2 < DenseViewpoints.size(); ++j)
    {
      const long long c = std::min(std::max(static_cast<long long>(j) - firstOrdinal, 0ll), n - 1);
      const double* T = corrections.data() + 16 * c;
      float* v = DenseViewpoints.data() + 3 * j;
      const double x = v[0], y = v[1], z = v[2];
      for (int a = 0; a < 3; ++a) v[a] = static_cast<float>(((T[4 * a] * x + T[4 * a + 1] * y) + T[4 * a + 2] * z) + T[4 * a + 3]);
    }
    return LSA_OK;
  }
  const std::string why = std::string("dense map: not re-projected, cleared: ") + lsa_last_error(Ctx);
  DropDenseMap("an applied trajectory whose re-projection failed");
  LastError = why;
  return rc == LSA_E_CAPACITY ? LSA_OK : rc;
}

int SlamCore::DenseReady(const char* who)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  if (DenseMapMode == 0)
  {
    LastError = std::string(who) + ": the dense map is off (set \"DenseMap\" to 1 or 2 before the frames)";
    return LSA_E_STATE;
  }
  WaitMaps();
  return LSA_OK;
}

int SlamCore::DenseMapSize()
{
  if (const int rc = DenseReady("DenseMapSize"); rc < 0) return rc;
  if (!Dense) return 0;
  const int n = lsa_dense_map_size(Dense);
  return n < 0 ? Fail(n, "lsa_dense_map_size") : n;
}

int SlamCore::GetDenseMap(int minFrames, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity)
{
  if (const int rc = DenseReady("GetDenseMap"); rc < 0) return rc;
  if (capacity < 0) { LastError = "GetDenseMap: bad argument"; return LSA_E_ARG; }
  if (!Dense) return 0;
  const int n = lsa_dense_map_get(Dense, minFrames, pts, voxels, capacity);
  return n < 0 ? Fail(n, "lsa_dense_map_get") : n;
}

int SlamCore::GetDenseMapSources(int minFrames, int* out, int capacity)
{
  if (const int rc = DenseReady("GetDenseMapSources"); rc < 0) return rc;
  if (capacity < 0) { LastError = "GetDenseMapSources: bad argument"; return LSA_E_ARG; }
  if (!Dense) return 0;
  const int n = lsa_dense_map_get_sources(Dense, minFrames, out, capacity);
  return n < 0 ? Fail(n, "lsa_dense_map_get_sources") : n;
}

int SlamCore::SaveDenseMapToPCD(const std::string& path, int format, int minFrames)
{
  if (const int rc = DenseReady("SaveDenseMapToPCD"); rc < 0) return rc;
  if (!Dense) return 0;  // an empty cloud is not saved
  const int n = lsa_dense_map_save_pcd(Dense, path.c_str(), format, minFrames);
  return n < 0 ? Fail(n, "lsa_dense_map_save_pcd") : n;
}

int SlamCore::SetDenseCarveParams()
{
  if (!Dense) return LSA_OK;
  if (const int rc = lsa_dense_map_set(Dense, "CarveRange", DenseMapCarveRange); rc < 0) return Fail(rc, "lsa_dense_map_set");
  if (const int rc = lsa_dense_map_set(Dense, "CarveMarginLeaves", DenseMapCarveMarginLeaves); rc < 0) return Fail(rc, "lsa_dense_map_set");
  if (const int rc = lsa_dense_map_set(Dense, "CarveStride", DenseMapCarveStride); rc < 0) return Fail(rc, "lsa_dense_map_set");
  return LSA_OK;
}

int SlamCore::GetDenseMapFiltered(int minFrames, double maxMissRatio, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity)
{
  if (const int rc = DenseReady("GetDenseMap"); rc < 0) return rc;
  if (capacity < 0) { LastError = "GetDenseMap: bad argument"; return LSA_E_ARG; }
  if (!Dense) return 0;
  const int n = lsa_dense_map_get_filtered(Dense, minFrames, maxMissRatio, pts, voxels, capacity);
  return n < 0 ? Fail(n, "lsa_dense_map_get_filtered") : n;
}

int SlamCore::GetDenseMapMisses(int minFrames, double maxMissRatio, uint32_t* out, int capacity)
{
  if (const int rc = DenseReady("GetDenseMapMisses"); rc < 0) return rc;
  if (capacity < 0) { LastError = "GetDenseMapMisses: bad argument"; return LSA_E_ARG; }
  if (!Dense) return 0;
  const int n = lsa_dense_map_get_misses(Dense, minFrames, maxMissRatio, out, capacity);
  return n < 0 ? Fail(n, "lsa_dense_map_get_misses") : n;
}

int SlamCore::SaveDenseMapToPCDFiltered(const std::string& path, int format, int minFrames, double maxMissRatio)
{
  if (const int rc = DenseReady("SaveDenseMapToPCD"); rc < 0) return rc;
  if (!Dense) return 0;  // an empty cloud is not saved
  const int n = lsa_dense_map_save_pcd_filtered(Dense, path.c_str(), format, minFrames, maxMissRatio);
  return n < 0 ? Fail(n, "lsa_dense_map_save_pcd_filtered") : n;
}

int SlamCore::PruneDenseMap(int minFrames, double maxMissRatio, long long* removed)
{
  if (const int rc = DenseReady("PruneDenseMap"); rc < 0) return rc;
  if (!removed) { LastError = "PruneDenseMap: bad argument"; return LSA_E_ARG; }
  *removed = 0;
  if (!Dense) return LSA_OK;
  const int rc = lsa_dense_map_prune(Dense, minFrames, maxMissRatio, removed);
  return rc < 0 ? Fail(rc, "lsa_dense_map_prune") : LSA_OK;
}

// per point of GetRegisteredFrame, in its order: where the sensor stood when it measured the point (float xyz)
int SlamCore::GetRegisteredFrameOrigins(std::vector<float>& out)
{
  if (!Ctx) return LSA_E_NO_DEVICE;
  out.clear();
  if (!HaveFrame) return 0;
  auto origins = [&](const Pose& offset, double timeOffset, float* xyz, int n) -> int {
    if (Undistortion)
    {
      const Pose H0 = (Tworld * Motion.GetH0()) * offset;
      const Pose H1 = (Tworld * Motion.GetH1()) * offset;
      return lsa_transform_frame_origins_at(Ctx, 1, H0.m, H1.m, Motion.Time0, Motion.Time1, timeOffset, xyz, n);
    }
    const Pose tf = Tworld * offset;
    return lsa_transform_frame_origins_at(Ctx, 0, tf.m, nullptr, 0., 0., timeOffset, xyz, n);
  };
  if (!CurrentFrames.empty())
  {
    size_t total = 0;
    for (const HeldFrame& f : CurrentFrames) total += static_cast<size_t>(f.n);
    out.resize(3 * total);
    size_t at = 0;
    for (const HeldFrame& f : CurrentFrames)
    {
      LSA_TRY(lsa_frame_store_use(Ctx, f.slot));
      LSA_TRY(origins(GetBaseToLidarOffset(f.device), f.timeOffset, out.data() + 3 * at, f.n));
      at += static_cast<size_t>(f.n);
    }
    return static_cast<int>(total);
  }
  const int n = lsa_frame_size(Ctx);
  if (n <= 0) return 0;
  out.resize(3 * static_cast<size_t>(n));
  LSA_TRY(origins(BaseToLidarOffset, 0., out.data(), n));
  return n;
}

int SlamCore::GetDenseMapNormals(int minFrames, double maxMissRatio, int radiusLeaves, int minNeighbors, int orient, lsa_dense_normal_t* out, int capacity)
{
  if (const int rc = DenseReady("GetDenseMapNormals"); rc < 0) return rc;
  if (capacity < 0) { LastError = "GetDenseMapNormals: bad argument"; return LSA_E_ARG; }
  if (!Dense) return 0;
  const int nv = orient ? static_cast<int>(DenseViewpoints.size() / 3) : 0;
  const int n = lsa_dense_map_get_normals(Dense, minFrames, maxMissRatio, radiusLeaves, minNeighbors, nv ? DenseViewpoints.data() : nullptr, nv, 0, out, capacity);
  return n < 0 ? Fail(n, "lsa_dense_map_get_normals") : n;
}

int SlamCore::SaveDenseMapToPCDNormals(const std::string& path, int format, int minFrames, double maxMissRatio, int radiusLeaves, int minNeighbors, int orient)
{
  if (const int rc = DenseReady("SaveDenseMapWithNormalsToPCD"); rc < 0) return rc;
  if (!Dense) return 0;  // an empty cloud is not saved
  const int nv = orient ? static_cast<int>(DenseViewpoints.size() / 3) : 0;
  const int n = lsa_dense_map_save_pcd_normals(Dense, path.c_str(), format, minFrames, maxMissRatio, radiusLeaves, minNeighbors, nv ? DenseViewpoints.data() : nullptr, nv, 0);
  return n < 0 ? Fail(n, "lsa_dense_map_save_pcd_normals") : n;
}

// per inserted ordinal since the last clear, float xyz; *firstFrame: the ordinal of entry 0
int SlamCore::GetDenseMapViewpoints(float* xyz, int capacity, int* firstFrame)
{
  if (const int rc = DenseReady("GetDenseMapViewpoints"); rc < 0) return rc;
  if (capacity < 0 || (capacity > 0 && !xyz)) { LastError = "GetDenseMapViewpoints: bad argument"; return LSA_E_ARG; }
  const int n = static_cast<int>(DenseViewpoints.size() / 3);
  if (firstFrame) *firstFrame = static_cast<int>(DenseFrames) - n;  // (0: what clears the map starts the ordinals again)
  const int take = std::min(n, capacity);
  if (take > 0) std::memcpy(xyz, DenseViewpoints.data(), static_cast<size_t>(take) * 3 * sizeof(float));
  return n;
}

// (a map no frame has reached yet is made here, empty: a window is answered whatever the map holds)
long long SlamCore::GetDenseMapGrid(const lsa_dense_grid_params_t* params, lsa_dense_grid_info_t* info, lsa_dense_cell_t* cells, int8_t* state, long long capacity)
{
  if (const int rc = DenseReady("GetDenseMapGrid"); rc < 0) return rc;
  if (!params || !info || capacity < 0) { LastError = "GetDenseMapGrid: bad argument"; return LSA_E_ARG; }
  if (const int rc = MakeDenseMap(); rc < 0) return rc;
  const long long n = lsa_dense_map_get_grid(Dense, params, info, cells, state, capacity);
  return n < 0 ? Fail(static_cast<int>(n), "lsa_dense_map_get_grid") : n;
}

long long SlamCore::SaveDenseMapGrid(const lsa_dense_grid_params_t* params, const std::string& prefix)
{
  if (const int rc = DenseReady("SaveDenseMapGrid"); rc < 0) return rc;
  if (!params) { LastError = "SaveDenseMapGrid: bad argument"; return LSA_E_ARG; }
  if (const int rc = MakeDenseMap(); rc < 0) return rc;
  const long long n = lsa_dense_map_save_grid(Dense, params, prefix.c_str());
  return n < 0 ? Fail(static_cast<int>(n), "lsa_dense_map_save_grid") : n;
}

// ---- rays (lsa_dense_cast.hip): each call behind WaitMaps, on a map that is made empty where no frame has reached it yet
int SlamCore::CastDenseMapRays(const float* origins, int nOrigins, const float* targets, int n, const lsa_dense_cast_params_t* params, lsa_dense_hit_t* hits, lsa_point_t* points)
{
  if (const int rc = DenseReady("CastDenseMapRays"); rc < 0) return rc;
  if (const int rc = MakeDenseMap(); rc < 0) return rc;
  const int rc = lsa_dense_map_cast(Dense, origins, nOrigins, targets, n, params, hits, points);
  return rc < 0 ? Fail(rc, "lsa_dense_map_cast") : rc;
}

// pose16 == nullptr: where the sensor stands now, Tworld * BaseToLidarOffset
int SlamCore::RenderDenseMapScan(const double* pose16, const double* elevations, int nRings, int nAzimuth, const lsa_dense_cast_params_t* params, lsa_dense_hit_t* hits)
{
  if (const int rc = DenseReady("RenderDenseMapScan"); rc < 0) return rc;
  if (!elevations || !hits || !params || nRings < 0 || nAzimuth < 0 || static_cast<long long>(nRings) * nAzimuth > (1ll << 30))
  {
    LastError = "RenderDenseMapScan: bad argument";
    return LSA_E_ARG;
  }
  if (const int rc = MakeDenseMap(); rc < 0) return rc;
  const Pose view = Tworld * BaseToLidarOffset;
  const int n = nRings * nAzimuth;
  float origin[3];
  std::vector<float> targets(3 * static_cast<size_t>(std::max(n, 1)));
  if (const int rc = lsa_scan_targets(pose16 ? pose16 : view.m, elevations, nRings, nAzimuth, origin, targets.data()); rc < 0)
  {
    LastError = "RenderDenseMapScan: bad argument";
    return rc;
  }
  const int rc = lsa_dense_map_cast(Dense, origin, 1, targets.data(), n, params, hits, nullptr);
  return rc < 0 ? Fail(rc, "lsa_dense_map_cast") : rc;
}

// one label per point of GetRegisteredFrame, in its order: every device frame of the last call with its own offset and time
// shift under the poses InsertDenseFrame and GetRegisteredFrameOrigins use
int SlamCore::CompareFrameToDenseMap(const lsa_dense_cast_params_t* params, uint8_t* labels, int capacity, long long counts[4])
{
  if (const int rc = DenseReady("CompareFrameToDenseMap"); rc < 0) return rc;
  if (!labels || !counts || capacity < 0) { LastError = "CompareFrameToDenseMap: bad argument"; return LSA_E_ARG; }
  lsa_dense_cast_params_t p;
  if (params) p = *params;
  else
  {
    std::memset(&p, 0, sizeof(p));
    p.max_range = 30.;
    p.extend = DenseMapLeafSize;  // the tolerance: one leaf
    p.max_miss_ratio = -1.;
    p.min_frames = 1;
    p.use_before = 2;
  }
  if (p.use_before == 2)
  {
    // automatic: the map as it stood before the call that brought this frame, when that call went into it
    p.use_before = DenseLastOrdinal >= 0 ? 1 : 0;
    p.before = DenseLastOrdinal >= 0 ? DenseLastOrdinal : 0;
  }
  if (const int rc = MakeDenseMap(); rc < 0) return rc;
  long long total = 0;
  if (HaveFrame)
  {
    if (!CurrentFrames.empty())
      for (const HeldFrame& f : CurrentFrames) total += f.n;
    else
      total = std::max(lsa_frame_size(Ctx), 0);
  }
  if (total > capacity) { LastError = "CompareFrameToDenseMap: the frame has more points than the labels have room for"; return LSA_E_CAPACITY; }
  long long sum[4] = {0, 0, 0, 0};
  if (total == 0)
  {
    // (no frame: the parameters are still held to their ranges)
    const float none[3] = {0.f, 0.f, 0.f};
    lsa_point_t nothing;
    std::memset(&nothing, 0, sizeof(nothing));
    const int rc = lsa_dense_map_compare_points(Dense, &nothing, 0, none, 1, &p, labels, sum);
    if (rc < 0) return Fail(rc, "lsa_dense_map_compare_points");
    std::memcpy(counts, sum, sizeof(sum));
    return 0;
  }
  auto compare = [&](const Pose& offset, double timeOffset, uint8_t* out, int room) -> int {
    long long c[4] = {0, 0, 0, 0};
    int rc;
    if (Undistortion)
    {
      const Pose H0 = (Tworld * Motion.GetH0()) * offset;
      const Pose H1 = (Tworld * Motion.GetH1()) * offset;
      rc = lsa_dense_map_compare_frame(Dense, 1, H0.m, H1.m, Motion.Time0, Motion.Time1, timeOffset, &p, out, room, c);
    }
    else
    {
      const Pose tf = Tworld * offset;
      rc = lsa_dense_map_compare_frame(Dense, 0, tf.m, nullptr, 0., 0., timeOffset, &p, out, room, c);
    }
    if (rc < 0) return Fail(rc, "lsa_dense_map_compare_frame");
    for (int l = 0; l < 4; ++l) sum[l] += c[l];
    return rc;
  };
  int at = 0;
  if (!CurrentFrames.empty())
  {
    for (const HeldFrame& f : CurrentFrames)
    {
      LSA_TRY(lsa_frame_store_use(Ctx, f.slot));
      const int got = compare(GetBaseToLidarOffset(f.device), f.timeOffset, labels + at, capacity - at);
      if (got < 0) return got;
      at += got;
    }
  }
  else
  {
    const int got = compare(BaseToLidarOffset, 0., labels, capacity);
    if (got < 0) return got;
    at = got;
  }
  std::memcpy(counts, sum, sizeof(sum));
  return at;
}

int SlamCore::ClearDenseMap()
{
  if (const int rc = DenseReady("ClearDenseMap"); rc < 0) return rc;
  DropDenseMap(nullptr);
  return LSA_OK;
}

}  // namespace host
}  // namespace lsa

// D_i = new_i * inverse(old_i) with the rigid inverse (R^T, -R^T t), in double: what moves a point placed under old_i to
// where new_i places it.  The pipeline's own numbers, for the callers and tests that hold lsa_dense_map_reproject to them.
extern "C" int lsa_pose_corrections(const double* old16, const double* new16, int n, double* out16)
{
  if (!old16 || !new16 || !out16 || n < 0) return LSA_E_ARG;
  for (int i = 0; i < n; ++i)
  {
    lsa::host::Pose a, b;
    std::memcpy(a.m, old16 + 16 * static_cast<size_t>(i), sizeof(a.m));
    std::memcpy(b.m, new16 + 16 * static_cast<size_t>(i), sizeof(b.m));
    const lsa::host::Pose d = b * lsa::host::Inverse(a);
    std::memcpy(out16 + 16 * static_cast<size_t>(i), d.m, sizeof(d.m));
  }
  return LSA_OK;
}
