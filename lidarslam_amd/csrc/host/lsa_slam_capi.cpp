// lsa_slam_capi.cpp -- pipeline-level C ABI (lsa_slam_*): LidarSlam::Slam behind a handle.
// Mirrors Slam::AddFrame / GetWorldTransform / GetKeypoints / GetRegisteredFrame
// (slam_lib/include/LidarSlam/Slam.h:111-178).
#include <algorithm>
#include <cstring>
#include "lsa_slam_core.h"

using lsa::host::SlamCore;

struct lsa_slam
{
  explicit lsa_slam(int device) : core(device) {}
  SlamCore core;
  std::vector<lsa_point_t> scratch;
  int map_io_counts[3] = {-1, -1, -1};  // points per type of the last lsa_slam_save_maps_pcd / lsa_slam_load_maps_pcd
};

extern "C" {

int lsa_slam_create(int device_id, lsa_slam** out)
{
  if (!out) return LSA_E_ARG;
  *out = nullptr;
  lsa_slam* s = new lsa_slam(device_id);
  if (!s->core.Ok())
  {
    delete s;
    return LSA_E_NO_DEVICE;  // loud failure: the device path is the only path
  }
  *out = s;
  return LSA_OK;
}

void lsa_slam_destroy(lsa_slam* s) { delete s; }

const char* lsa_slam_last_error(const lsa_slam* s) { return s ? s->core.Error().c_str() : "null handle"; }

int lsa_slam_set_param(lsa_slam* s, const char* name, double value)
{
  if (!s || !name) return LSA_E_ARG;
  return s->core.SetParam(name, value);
}

int lsa_slam_get_param(const lsa_slam* s, const char* name, double* value)
{
  if (!s || !name) return LSA_E_ARG;
  return s->core.GetParam(name, value);
}

int lsa_slam_add_wheel_odom_measurement(lsa_slam* s, double time, double distance)
{
  if (!s) return LSA_E_ARG;
  s->core.Sensors().AddWheelOdom(time, distance);
  return LSA_OK;
}

int lsa_slam_add_gravity_measurement(lsa_slam* s, double time, const double acc[3])
{
  if (!s || !acc) return LSA_E_ARG;
  s->core.Sensors().AddGravity(time, acc);
  return LSA_OK;
}

int lsa_slam_clear_sensor_measurements(lsa_slam* s)
{
  if (!s) return LSA_E_ARG;
  s->core.Sensors().Clear();
  return LSA_OK;
}

int lsa_slam_sensor_terms(const lsa_slam* s, lsa_sensor_terms_t* out)
{
  if (!s || !out) return LSA_E_ARG;
  *out = s->core.LocalizationSensorTerms();
  return LSA_OK;
}

void lsa_slam_reset(lsa_slam* s, int reset_log)
{
  if (s) s->core.Reset(reset_log != 0);
}

int lsa_slam_add_frame(lsa_slam* s, const lsa_point_t* pts, int n, uint64_t stamp_us, uint32_t seq)
{
  if (!s) return LSA_E_ARG;
  return s->core.AddFrame(pts, n, stamp_us, seq);
}

int lsa_slam_store_frame(lsa_slam* s, int slot, const lsa_point_t* pts, int n)
{
  if (!s) return LSA_E_ARG;
  return lsa_frame_store_put(s->core.Context(), slot, pts, n);
}

int lsa_slam_add_stored_frame(lsa_slam* s, int slot, uint64_t stamp_us, uint32_t seq)
{
  if (!s) return LSA_E_ARG;
  return s->core.AddStoredFrame(slot, stamp_us, seq);
}

int lsa_slam_get_world_transform(const lsa_slam* s, double T[16], double* time)
{
  if (!s || !T) return LSA_E_ARG;
  const lsa::host::Pose p = s->core.GetWorldTransform(time);
  std::memcpy(T, p.m, sizeof(p.m));
  return LSA_OK;
}

int lsa_slam_get_covariance(const lsa_slam* s, double cov[36])
{
  if (!s || !cov) return LSA_E_ARG;
  std::memcpy(cov, s->core.GetTransformCovariance().data(), 36 * sizeof(double));
  return LSA_OK;
}

int lsa_slam_get_keypoints(lsa_slam* s, int type, int which, lsa_point_t* out, int capacity)
{
  if (!s || type < 0 || type > 2 || (!out && capacity > 0)) return LSA_E_ARG;
  int n = which == 2 ? s->core.GetRawKeypoints(type, s->scratch) : s->core.GetKeypoints(type, which == 1, s->scratch);
  if (n < 0) return n;
  n = std::min(n, capacity);
  if (n > 0) std::memcpy(out, s->scratch.data(), (size_t)n * sizeof(lsa_point_t));
  return n;
}

int lsa_slam_get_registered_frame(lsa_slam* s, lsa_point_t* out, int capacity)
{
  if (!s || (!out && capacity > 0)) return LSA_E_ARG;
  int n = s->core.GetRegisteredFrame(s->scratch);
  if (n < 0) return n;
  n = std::min(n, capacity);
  if (n > 0) std::memcpy(out, s->scratch.data(), (size_t)n * sizeof(lsa_point_t));
  return n;
}

int lsa_slam_get_match_status(lsa_slam* s, int localization, int type, uint8_t* status, double* weights, int capacity)
{
  if (!s || type < 0 || type > 2) return LSA_E_ARG;
  const lsa::host::MatchDebug& d = s->core.GetMatchDebug(localization != 0, type);
  const int n = std::min<int>(capacity, d.status.size());
  if (n > 0 && status) std::memcpy(status, d.status.data(), n);
  if (n > 0 && weights) std::memcpy(weights, d.weights.data(), (size_t)n * sizeof(double));
  return n;
}

int lsa_slam_get_stats(const lsa_slam* s, double out[16])
{
  if (!s || !out) return LSA_E_ARG;
  const lsa::host::FrameStats& t = s->core.Stats;
  const double v[16] = {t.total, t.extract, t.ego_icp, t.ego_lm, t.loc_icp, t.loc_lm, t.undistort, t.submap, t.maps,
                        (double)t.ego_iters, (double)t.loc_iters, (double)t.lm_evals, (double)s->core.TotalMatchedKeypoints,
                        (double)s->core.KfCounter, t.maps_wait, t.maps_async};
  std::memcpy(out, v, sizeof(v));
  return LSA_OK;
}

// ---- the remaining result getters of Slam.h:141-189 ----
int lsa_slam_get_latency_compensated_world_transform(const lsa_slam* s, double T[16], double* time)
{
  if (!s || !T) return LSA_E_ARG;
  const lsa::host::Pose p = s->core.GetLatencyCompensatedWorldTransform(time);
  std::memcpy(T, p.m, sizeof(p.m));
  return LSA_OK;
}

int lsa_slam_set_base_to_lidar_offset(lsa_slam* s, const double T[16], int device_id)
{
  if (!s || !T) return LSA_E_ARG;
  lsa::host::Pose p;
  std::memcpy(p.m, T, sizeof(p.m));
  return s->core.SetBaseToLidarOffset(device_id, p);
}

int lsa_slam_get_base_to_lidar_offset(const lsa_slam* s, double T[16], int device_id)
{
  if (!s || !T || device_id < 0 || device_id > 255) return LSA_E_ARG;
  const lsa::host::Pose p = s->core.GetBaseToLidarOffset(device_id);
  std::memcpy(T, p.m, sizeof(p.m));
  return LSA_OK;
}

int lsa_slam_hint_next_stored_frame(lsa_slam* s, int slot)
{
  if (!s) return LSA_E_ARG;
  s->core.HintNextStoredFrame(slot);
  return LSA_OK;
}

int lsa_slam_clear_maps(lsa_slam* s)
{
  if (!s) return LSA_E_ARG;
  s->core.ClearMaps();
  return LSA_OK;
}

int lsa_slam_hint_next_frame(lsa_slam* s, const lsa_point_t* pts, int n)
{
  if (!s) return LSA_E_ARG;
  return s->core.HintNextFrame(pts, n);
}

int lsa_slam_set_extractor_param(lsa_slam* s, int device_id, const char* name, double value)
{
  if (!s || !name) return LSA_E_ARG;
  return s->core.SetExtractorParam(device_id, name, value);
}

int lsa_slam_get_extractor_param(const lsa_slam* s, int device_id, const char* name, double* value)
{
  if (!s || !name) return LSA_E_ARG;
  return s->core.GetExtractorParam(device_id, name, value);
}

int lsa_slam_add_frames(lsa_slam* s, const lsa_point_t* const* pts, const int* n, const uint64_t* stamp_us, const uint32_t* seq, int nframes)
{
  if (!s || !pts || !n || !stamp_us || nframes <= 0 || nframes > 16) return LSA_E_ARG;
  lsa::host::SlamCore::InputFrame frames[16];
  for (int i = 0; i < nframes; ++i) frames[i] = {pts[i], n[i], stamp_us[i], seq ? seq[i] : 0u};
  return s->core.AddFrames(frames, nframes);
}

int lsa_slam_set_world_transform_from_guess(lsa_slam* s, const double T[16])
{
  if (!s || !T) return LSA_E_ARG;
  lsa::host::Pose p;
  std::memcpy(p.m, T, sizeof(p.m));
  return s->core.SetWorldTransformFromGuess(p);
}

int lsa_slam_get_trajectory(const lsa_slam* s, double* poses, double* covariances, int capacity)
{
  if (!s || capacity < 0) return LSA_E_ARG;
  const auto& traj = s->core.LogTrajectory;
  const auto& covs = s->core.LogCovariances;
  const int n = static_cast<int>(traj.size());
  for (int i = 0; i < std::min(n, capacity); ++i)
  {
    if (poses)
    {
      std::memcpy(poses + 17 * i, traj[i].pose.m, 16 * sizeof(double));
      poses[17 * i + 16] = traj[i].time;
    }
    if (covariances)
    {
      // the covariances are logged only while LoggingTimeout != 0, newest last like the poses
      const long j = static_cast<long>(covs.size()) - n + i;
      if (j >= 0) std::memcpy(covariances + 36 * i, covs[j].data(), 36 * sizeof(double));
      else std::memset(covariances + 36 * i, 0, 36 * sizeof(double));
    }
  }
  return n;
}

int lsa_slam_get_debug_information(lsa_slam* s, double out[10])
{
  if (!s || !out) return LSA_E_ARG;
  return s->core.GetDebugInformation(out);
}

int lsa_slam_get_map(lsa_slam* s, int type, int clean, lsa_point_t* out, int capacity)
{
  if (!s || type < 0 || type > 2 || capacity < 0 || (capacity > 0 && !out)) return LSA_E_ARG;
  std::vector<lsa_point_t> pc;
  const int n = s->core.GetMap(type, clean != 0, pc);
  if (n < 0) return n;
  if (std::min(n, capacity) > 0) std::memcpy(out, pc.data(), static_cast<size_t>(std::min(n, capacity)) * sizeof(lsa_point_t));
  return n;
}

int lsa_slam_get_target_submap(lsa_slam* s, int type, lsa_point_t* out, int capacity)
{
  if (!s || type < 0 || type > 2 || capacity < 0 || (capacity > 0 && !out)) return LSA_E_ARG;
  std::vector<lsa_point_t> pc;
  const int n = s->core.GetTargetSubMap(type, pc);
  if (n < 0) return n;
  if (std::min(n, capacity) > 0) std::memcpy(out, pc.data(), static_cast<size_t>(std::min(n, capacity)) * sizeof(lsa_point_t));
  return n;
}

lsa_ctx* lsa_slam_context(lsa_slam* s) { return s ? s->core.Context() : nullptr; }

// ---- Slam::SaveMapsToPCD / LoadMapsFromPCD (Slam.cxx:504-543) and the primitive under the loader ----
int lsa_slam_add_map_points(lsa_slam* s, int type, const lsa_point_t* pts, int n, int fixed, double time)
{
  if (!s) return LSA_E_ARG;
  return s->core.AddMapPoints(type, pts, n, fixed != 0, time);
}

int lsa_slam_save_maps_pcd(lsa_slam* s, const char* prefix, int format, int filtered)
{
  if (!s || !prefix) return LSA_E_ARG;
  return s->core.SaveMapsToPCD(prefix, format, filtered != 0, s->map_io_counts);
}

int lsa_slam_load_maps_pcd(lsa_slam* s, const char* prefix, int reset_maps, double time)
{
  if (!s || !prefix) return LSA_E_ARG;
  return s->core.LoadMapsFromPCD(prefix, reset_maps != 0, time, s->map_io_counts);
}

int lsa_slam_map_io_counts(const lsa_slam* s, int counts[3])
{
  if (!s || !counts) return LSA_E_ARG;
  std::memcpy(counts, s->map_io_counts, sizeof(s->map_io_counts));
  return LSA_OK;
}

// ---- the dense point-cloud map (lsa_slam_dense.cpp) ----
int lsa_slam_dense_map_size(lsa_slam* s) { return s ? s->core.DenseMapSize() : LSA_E_ARG; }

int lsa_slam_get_dense_map(lsa_slam* s, int min_frames, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.GetDenseMap(min_frames, pts, voxels, capacity);
}

int lsa_slam_get_dense_map_sources(lsa_slam* s, int min_frames, int* out, int capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.GetDenseMapSources(min_frames, out, capacity);
}

int lsa_slam_save_dense_map_pcd(lsa_slam* s, const char* path, int format, int min_frames)
{
  if (!s || !path) return LSA_E_ARG;
  return s->core.SaveDenseMapToPCD(path, format, min_frames);
}

int lsa_slam_clear_dense_map(lsa_slam* s) { return s ? s->core.ClearDenseMap() : LSA_E_ARG; }

int lsa_slam_get_dense_map_filtered(lsa_slam* s, int min_frames, double max_miss_ratio, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.GetDenseMapFiltered(min_frames, max_miss_ratio, pts, voxels, capacity);
}

int lsa_slam_get_dense_map_misses(lsa_slam* s, int min_frames, double max_miss_ratio, uint32_t* out, int capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.GetDenseMapMisses(min_frames, max_miss_ratio, out, capacity);
}

int lsa_slam_save_dense_map_pcd_filtered(lsa_slam* s, const char* path, int format, int min_frames, double max_miss_ratio)
{
  if (!s || !path) return LSA_E_ARG;
  return s->core.SaveDenseMapToPCDFiltered(path, format, min_frames, max_miss_ratio);
}

int lsa_slam_prune_dense_map(lsa_slam* s, int min_frames, double max_miss_ratio, long long* removed)
{
  if (!s) return LSA_E_ARG;
  return s->core.PruneDenseMap(min_frames, max_miss_ratio, removed);
}

int lsa_slam_get_dense_map_normals(lsa_slam* s, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors, int orient, lsa_dense_normal_t* out, int capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.GetDenseMapNormals(min_frames, max_miss_ratio, radius_leaves, min_neighbors, orient, out, capacity);
}

int lsa_slam_save_dense_map_pcd_normals(lsa_slam* s, const char* path, int format, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors, int orient)
{
  if (!s || !path) return LSA_E_ARG;
  return s->core.SaveDenseMapToPCDNormals(path, format, min_frames, max_miss_ratio, radius_leaves, min_neighbors, orient);
}

int lsa_slam_get_dense_map_viewpoints(lsa_slam* s, float* xyz, int capacity, int* first_frame)
{
  if (!s) return LSA_E_ARG;
  return s->core.GetDenseMapViewpoints(xyz, capacity, first_frame);
}

long long lsa_slam_get_dense_map_grid(lsa_slam* s, const lsa_dense_grid_params_t* params, lsa_dense_grid_info_t* info, lsa_dense_cell_t* cells, int8_t* state,
                                      long long capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.GetDenseMapGrid(params, info, cells, state, capacity);
}

long long lsa_slam_save_dense_map_grid(lsa_slam* s, const lsa_dense_grid_params_t* params, const char* prefix)
{
  if (!s || !prefix) return LSA_E_ARG;
  return s->core.SaveDenseMapGrid(params, prefix);
}

int lsa_slam_cast_dense_map_rays(lsa_slam* s, const float* origins_xyz, int n_origins, const float* targets_xyz, int n, const lsa_dense_cast_params_t* params,
                                 lsa_dense_hit_t* hits, lsa_point_t* points)
{
  if (!s) return LSA_E_ARG;
  return s->core.CastDenseMapRays(origins_xyz, n_origins, targets_xyz, n, params, hits, points);
}

int lsa_slam_render_dense_map_scan(lsa_slam* s, const double* pose16, const double* elevations_rad, int n_rings, int n_azimuth, const lsa_dense_cast_params_t* params,
                                   lsa_dense_hit_t* hits)
{
  if (!s) return LSA_E_ARG;
  return s->core.RenderDenseMapScan(pose16, elevations_rad, n_rings, n_azimuth, params, hits);
}

int lsa_slam_compare_frame_to_dense_map(lsa_slam* s, const lsa_dense_cast_params_t* params, uint8_t* labels, int capacity, long long counts[4])
{
  if (!s) return LSA_E_ARG;
  return s->core.CompareFrameToDenseMap(params, labels, capacity, counts);
}

int lsa_slam_get_registered_frame_origins(lsa_slam* s, float* xyz, int capacity)
{
  if (!s || (!xyz && capacity > 0)) return LSA_E_ARG;
  std::vector<float> origins;
  int n = s->core.GetRegisteredFrameOrigins(origins);
  if (n < 0) return n;
  n = std::min(n, capacity);
  if (n > 0) std::memcpy(xyz, origins.data(), (size_t)n * 3 * sizeof(float));
  return n;
}

// ---- a corrected trajectory brought back: what Slam::RunPoseGraphOptimization does after its optimizer (Slam.cxx:404-477) ----
int lsa_slam_set_trajectory_and_rebuild_maps(lsa_slam* s, const double* poses17, int n)
{
  if (!s) return LSA_E_ARG;
  return s->core.SetTrajectoryAndRebuildMaps(poses17, n);
}

int lsa_slam_logged_frames(const lsa_slam* s) { return s ? s->core.LoggedFrames() : LSA_E_ARG; }

int lsa_slam_get_logged_keypoints(lsa_slam* s, int frame, int type, lsa_point_t* out, int capacity)
{
  if (!s || capacity < 0 || (capacity > 0 && !out)) return LSA_E_ARG;
  const int n = s->core.GetLoggedKeypoints(frame, type, s->scratch);
  if (n < 0) return n;
  if (std::min(n, capacity) > 0) std::memcpy(out, s->scratch.data(), static_cast<size_t>(std::min(n, capacity)) * sizeof(lsa_point_t));
  return n;
}

void lsa_loop_closure_params_init(lsa_loop_closure_params_t* params)
{
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->revisited_half_window = 5;
}

int lsa_slam_register_logged_frames(lsa_slam* s, int query, int revisited, const lsa_loop_closure_params_t* params, const double guess[16],
                                    lsa_loop_closure_result_t* out)
{
  if (!s) return LSA_E_ARG;
  return s->core.RegisterLoggedFrames(query, revisited, params, guess, out);
}

int lsa_slam_recognize_place(lsa_slam* s, int query, const lsa_place_search_t* search, lsa_place_candidate_t* out, int capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.RecognizePlace(query, search, out, capacity);
}

int lsa_slam_detect_loop_closures(lsa_slam* s, const lsa_loop_detect_t* detect, lsa_loop_candidate_t* out, int capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.DetectLoopClosures(detect, out, capacity);
}

int lsa_slam_close_loops(lsa_slam* s, const lsa_loop_detect_t* detect, const lsa_loop_closure_params_t* loop_params, const lsa_pgo_params_t* pgo_params,
                         const lsa_pgo_robust_t* robust, double* poses17_out, int capacity, lsa_pgo_result_t* result, lsa_loop_report_t* reports_out,
                         int report_capacity)
{
  if (!s) return LSA_E_ARG;
  return s->core.CloseLoops(detect, loop_params, pgo_params, robust, poses17_out, capacity, result, reports_out, report_capacity);
}

int lsa_slam_recognize_place_in_maps(lsa_slam* s, const double* viewpoints, int V, const lsa_map_place_search_t* search, lsa_map_place_candidate_t* out, int capacity,
                                     lsa_map_place_summary_t* summary)
{
  if (!s) return LSA_E_ARG;
  return s->core.RecognizePlaceInMaps(viewpoints, V, search, out, capacity, summary);
}

int lsa_slam_optimize_logged_trajectory(lsa_slam* s, const lsa_pgo_edge_t* loop_edges, int m, const lsa_pgo_params_t* params, double* poses17_out, int capacity,
                                        lsa_pgo_result_t* result)
{
  if (!s) return LSA_E_ARG;
  return lsa_slam_optimize_logged_trajectory_robust(s, loop_edges, m, params, nullptr, poses17_out, capacity, result, nullptr);
}

int lsa_slam_optimize_logged_trajectory_robust(lsa_slam* s, const lsa_pgo_edge_t* loop_edges, int m, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust,
                                               double* poses17_out, int capacity, lsa_pgo_result_t* result, double* loop_verdict_out)
{
  if (!s) return LSA_E_ARG;
  return s->core.OptimizeLoggedTrajectory(loop_edges, m, params, poses17_out, capacity, result, robust, loop_verdict_out);
}

int lsa_slam_run_pose_graph_optimization(lsa_slam* s, const double* gps_times, const double* gps_xyz, const double* gps_cov9, int G, double* gps_to_sensor16,
                                         double time_offset, const lsa_pgo_params_t* params, double* poses17_out, int capacity, lsa_pgo_result_t* result)
{
  if (!s) return LSA_E_ARG;
  return lsa_slam_run_pose_graph_optimization_robust(s, gps_times, gps_xyz, gps_cov9, G, gps_to_sensor16, time_offset, params, nullptr, poses17_out, capacity, result, nullptr);
}

int lsa_slam_run_pose_graph_optimization_robust(lsa_slam* s, const double* gps_times, const double* gps_xyz, const double* gps_cov9, int G, double* gps_to_sensor16,
                                                double time_offset, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust, double* poses17_out, int capacity,
                                                lsa_pgo_result_t* result, double* fix_verdict_out)
{
  if (!s) return LSA_E_ARG;
  return s->core.RunPoseGraphOptimization(gps_times, gps_xyz, gps_cov9, G, gps_to_sensor16, time_offset, params, poses17_out, capacity, result, robust, fix_verdict_out);
}

int lsa_loop_closure_candidate(const double* poses17, int n, int query, double min_travelled, double max_distance)
{
  return lsa::host::LoopClosureCandidate(poses17, n, query, min_travelled, max_distance);
}

// ---- LidarSlam::RollingGrid on its own (include/lidarslam_amd.h, "the rolling voxel map") ----
struct lsa_rolling_grid
{
  lsa::host::RollingGrid grid;
};

lsa_rolling_grid* lsa_rolling_grid_create(void) { return new (std::nothrow) lsa_rolling_grid; }
void lsa_rolling_grid_destroy(lsa_rolling_grid* g) { delete g; }
int lsa_rolling_grid_set(lsa_rolling_grid* g, const char* name, double value)
{
  if (!g || !name) return LSA_E_ARG;
  const std::string n(name);
  if (n == "GridSize") g->grid.SetGridSize(static_cast<int>(value));
  else if (n == "VoxelResolution") g->grid.SetVoxelResolution(value);
  else if (n == "LeafSize") g->grid.SetLeafSize(value);
  else if (n == "MinFramesPerVoxel") g->grid.SetMinFramesPerVoxel(static_cast<unsigned int>(value));
  else if (n == "Sampling")
  {
    if (value < 0 || value > 4) return LSA_E_ARG;
    g->grid.SetSampling(static_cast<lsa::host::SamplingMode>(static_cast<int>(value)));
  }
  else if (n == "DecayingThreshold") g->grid.SetDecayingThreshold(value);
  else if (n == "AddThreads") g->grid.SetAddThreads(static_cast<int>(value));
  else if (n == "Ordered") g->grid.SetOrdered(value != 0);
  else return LSA_E_ARG;
  return LSA_OK;
}
void lsa_rolling_grid_reset(lsa_rolling_grid* g, const float position[3]) { if (g) g->grid.Reset(position); }
void lsa_rolling_grid_clear(lsa_rolling_grid* g) { if (g) g->grid.Clear(); }
int lsa_rolling_grid_size(const lsa_rolling_grid* g) { return g ? static_cast<int>(g->grid.Size()) : LSA_E_ARG; }
void lsa_rolling_grid_roll(lsa_rolling_grid* g, const float min_point[3], const float max_point[3])
{
  if (g && min_point && max_point) g->grid.Roll(min_point, max_point);
}
int lsa_rolling_grid_add(lsa_rolling_grid* g, const lsa_point_t* pts, int n, int fixed, double current_time, int roll)
{
  if (!g || n < 0 || (n > 0 && !pts)) return LSA_E_ARG;
  g->grid.Add(pts, static_cast<std::size_t>(n), fixed != 0, current_time, roll != 0);
  return LSA_OK;
}
void lsa_rolling_grid_clear_old_points(lsa_rolling_grid* g, double current_time) { if (g) g->grid.ClearOldPoints(current_time); }
int lsa_rolling_grid_get(const lsa_rolling_grid* g, int clean, lsa_point_t* out, int capacity)
{
  if (!g || capacity < 0 || (capacity > 0 && !out)) return LSA_E_ARG;
  const lsa::host::RollingGrid::PointCloud pc = g->grid.Get(clean != 0);
  const int n = std::min<int>(capacity, static_cast<int>(pc.size()));
  if (n > 0) std::memcpy(out, pc.data(), static_cast<std::size_t>(n) * sizeof(lsa_point_t));
  return n;
}
int lsa_rolling_grid_build_submap(lsa_rolling_grid* g, const float min_point[3], const float max_point[3], int min_nb_points)
{
  if (!g || ((min_point == nullptr) != (max_point == nullptr))) return LSA_E_ARG;
  if (min_point) g->grid.BuildSubMap(min_point, max_point, min_nb_points);
  else g->grid.BuildSubMap();
  return static_cast<int>(g->grid.SubMapSize());
}
int lsa_rolling_grid_submap_valid(const lsa_rolling_grid* g) { return g && g->grid.IsSubMapValid() ? 1 : 0; }
int lsa_rolling_grid_submap(const lsa_rolling_grid* g, lsa_point_t* out, int capacity)
{
  if (!g || capacity < 0 || (capacity > 0 && !out)) return LSA_E_ARG;
  const int n = std::min<int>(capacity, static_cast<int>(g->grid.SubMapSize()));
  if (n > 0) std::memcpy(out, g->grid.SubMapData(), static_cast<std::size_t>(n) * sizeof(lsa_point_t));
  return n;
}

}  // extern "C"
