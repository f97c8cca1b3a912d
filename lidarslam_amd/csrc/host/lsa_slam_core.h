// lsa_slam_core.h -- per-frame pipeline of LidarSlam::Slam on top of the C ABI
// (slam_lib/src/Slam.cxx: AddFrames :230-344, ExtractKeypoints :746-810, ComputeEgoMotion
//  :813-972, Localization :975-1175, UpdateMapsUsingTworld :1178-1222, LogCurrentFrameState
//  :1225-1264, undistortion :1271-1352; defaults slam_lib/include/LidarSlam/Slam.h:403-694).
//
// Host keeps what SURVEY.md 8 leaves on the host: frame checks, pose bookkeeping, the
// 6-dof trust-region control flow, the rolling voxel maps.  Everything per point / per
// keypoint runs on the device through lidarslam_amd.h.
//
// One class, one unit per job: lsa_slam_core.cpp (construction, the frame path, the look-ahead, the getters),
// lsa_slam_icp.cpp (the two registrations; their loop is lsa_slam_icp_loop.h), lsa_slam_maps.cpp (sub-maps, speculation,
// insertion, load / save), lsa_slam_log.cpp (the keypoint log and the calls on it), lsa_slam_dense.cpp (the dense point-cloud
// map), lsa_slam_params.cpp (parameters by name).
#pragma once
#include <array>
#include <atomic>
#include <deque>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <vector>
#include "../../../include/lidarslam_amd.h"
#include "lsa_host_worker.h"
#include "lsa_hostmath.h"
#include "lsa_lm.h"
#include "lsa_loop_closure.h"
#include "lsa_place.h"
#include "lsa_rolling_grid.h"
#include "lsa_sensor_constraints.h"

namespace lsa
{
namespace host
{

enum UndistortionMode { UNDISTORTION_NONE = 0, UNDISTORTION_ONCE = 1, UNDISTORTION_REFINED = 2 };
enum class EgoMotionMode { NONE = 0, MOTION_EXTRAPOLATION = 1, REGISTRATION = 2, MOTION_EXTRAPOLATION_AND_REGISTRATION = 3 };
enum class MappingMode { NONE = 0, ADD_KPTS_TO_FIXED_MAP = 1, UPDATE = 2 };

struct StampedPose
{
  Pose pose;
  double time;
};

struct FrameStats
{
  double total = 0, extract = 0, ego_icp = 0, ego_lm = 0, loc_icp = 0, loc_lm = 0, undistort = 0, submap = 0, maps = 0;
  int ego_iters = 0, loc_iters = 0, lm_evals = 0;
  int submap_spec_hits = 0;  // sub-maps extracted ahead of time that Localization() could keep
  double maps_wait = 0;   // time this frame waited for the previous keyframe's map insertion
  double maps_async = 0;  // duration of that insertion on the worker thread
};

struct MatchDebug
{
  std::vector<uint8_t> status;
  std::vector<double> weights;
};

class SlamCore
{
public:
  explicit SlamCore(int device);
  ~SlamCore();
  SlamCore(const SlamCore&) = delete;
  SlamCore& operator=(const SlamCore&) = delete;

  bool Ok() const { return Ctx != nullptr; }
  const std::string& Error() const { return LastError; }
  lsa_ctx* Context() { return Ctx; }

  // keepDenseMap: SetTrajectoryAndRebuildMaps' alone, when the dense map is re-projected instead of cleared
  void Reset(bool resetLog = true, bool keepDenseMap = false);
  // Slam::AddFrame on a host scan / on a scan resident in the frame store
  int AddFrame(const lsa_point_t* pts, int n, uint64_t stampUs, uint32_t seq);
  int AddStoredFrame(int slot, uint64_t stampUs, uint32_t seq);
  // Replay: the frame-store slot of the frame that will be added next.  Its keypoints are then extracted beside
  // the registration of the current frame (lsa_extract_prefetch) and the next AddStoredFrame finds them ready.
  // Slam::ClearMaps (Slam.cxx:1639-1643)
  void ClearMaps()
  {
    WaitMaps();
    for (auto& m : LocalMaps) m->Reset();
    for (auto* g : DevMaps)
      if (g) lsa_device_grid_reset(g, nullptr);
    DropDenseMap("ClearMaps");
  }
  // Points put into the map of one keypoint type: RollingGrid::Add(pts, fixed, time) with its default roll = true.  What
  // the map loader sits on; waits for the map workers and drops what the look-ahead had prepared from the maps as they were.
  int AddMapPoints(int type, const lsa_point_t* pts, int n, bool fixed, double time);
  // Slam::SaveMapsToPCD / LoadMapsFromPCD (Slam.cxx:504-543).  counts[k]: points written / read per type, -1 where no file
  // was written (type not in use, empty map) or found.  time < 0: the wall clock in whole seconds (std::time(nullptr)).
  int SaveMapsToPCD(const std::string& prefix, int format, bool filtered, int counts[3]);
  int LoadMapsFromPCD(const std::string& prefix, bool resetMaps, double time, int counts[3]);
  // What Slam::RunPoseGraphOptimization does after its optimizer (Slam.cxx:404-477): the logged poses replaced by poses17
  // (rows of lsa_slam_get_trajectory), the maps rebuilt from the keypoint log under them, Tworld / PreviousTworld set.
  int SetTrajectoryAndRebuildMaps(const double* poses17, int n);
  // Loop closure: logged frame `query` registered against the logged keypoints around `revisited` (lsa_slam_register_logged_frames
  // in lidarslam_amd.h says what it computes).  Everything runs on a scratch context of this object's: the frame path's
  // keypoint sets, targets, maps and look-ahead do not notice.  A refusal changes nothing and leaves its reason in Error().
  int RegisterLoggedFrames(int query, int revisited, const lsa_loop_closure_params_t* params, const double* guess16, lsa_loop_closure_result_t* out);
  // Place recognition: the logged frames before `query` that look like it, by the descriptors of the keypoint log
  // (lsa_slam_recognize_place in lidarslam_amd.h).  Runs on the log's context after the map workers; reads the log, writes
  // the log's descriptor store and nothing else.  Returns the number of candidates written.
  int RecognizePlace(int query, const lsa_place_search_t* search, lsa_place_candidate_t* out, int capacity);
  // Loop detection over the whole log: RecognizePlace for every query of a set in one pass on the device
  // (lsa_slam_detect_loop_closures in lidarslam_amd.h).  Refuses, waits and runs as RecognizePlace does.
  int DetectLoopClosures(const lsa_loop_detect_t* detect, lsa_loop_candidate_t* out, int capacity);
  // Detect, register every candidate, solve under the robust loss, apply where asked: the composition of DetectLoopClosures,
  // RegisterLoggedFrames and OptimizeLoggedTrajectory (lsa_slam_close_loops in lidarslam_amd.h).  Returns the number of reports.
  int CloseLoops(const lsa_loop_detect_t* detect, const lsa_loop_closure_params_t* loopParams, const lsa_pgo_params_t* pgoParams, const lsa_pgo_robust_t* robust,
                 double* poses17, int capacity, lsa_pgo_result_t* result, lsa_loop_report_t* reports, int reportCapacity);
  // Place recognition against the maps: the viewpoints from which the maps look like the last frame (lsa_slam_recognize_place_in_maps
  // in lidarslam_amd.h).  Runs after the map workers; reads the maps and the raw keypoints, writes the context's table of map
  // descriptors and nothing else; the pose is the caller's to set (SetWorldTransformFromGuess(candidate.guess)).  A refusal
  // changes nothing and leaves its reason in Error().
  int RecognizePlaceInMaps(const double* viewpoints, int V, const lsa_map_place_search_t* search, lsa_map_place_candidate_t* out, int capacity,
                           lsa_map_place_summary_t* summary);
  // Pose-graph optimization of the logged trajectory with the caller's loop edges (lsa_slam_optimize_logged_trajectory in
  // lidarslam_amd.h): the solve runs on the scratch context; with params->apply the result goes through
  // SetTrajectoryAndRebuildMaps, without it nothing of the frame path is touched.  Returns the number of poses.
  // robust: the loss on the caller's loop edges (NULL: none; the odometry chain is never discounted); loopVerdict: 2 m doubles or NULL
  int OptimizeLoggedTrajectory(const lsa_pgo_edge_t* loopEdges, int m, const lsa_pgo_params_t* params, double* poses17, int capacity, lsa_pgo_result_t* result,
                               const lsa_pgo_robust_t* robust = nullptr, double* loopVerdict = nullptr);
  // Slam::RunPoseGraphOptimization (lsa_slam_run_pose_graph_optimization in lidarslam_amd.h): GPS fixes matched to the logged
  // poses by time become position priors on a graph of free poses; solved on the scratch context from the track laid onto
  // the fixes, brought back onto logged pose 0.  gpsToSensor16: in the calibration, out the optimized pose 0 in the GPS frame.
  int RunPoseGraphOptimization(const double* gpsTimes, const double* gpsXyz, const double* gpsCov9, int G, double* gpsToSensor16, double timeOffset,
                               const lsa_pgo_params_t* params, double* poses17, int capacity, lsa_pgo_result_t* result, const lsa_pgo_robust_t* robust = nullptr,
                               double* fixVerdict = nullptr);  // robust: the loss on the GPS priors; fixVerdict: 2 G doubles or NULL, weight -1 = unmatched
  int LoggedFrames() const;
  int GetLoggedKeypoints(int frame, int type, std::vector<lsa_point_t>& out);
  void HintNextStoredFrame(int slot) { NextStoredSlot = slot; }
  // Replay from host clouds: the cloud of the AddFrame call after the next one.  Its upload starts at once (pinned
  // staging, copy stream, a thread of its own), its keypoints are extracted beside the registration of the frame in
  // between; AddFrame adopts both when it is handed this very cloud.  The cloud must stay valid until then.
  int HintNextFrame(const lsa_point_t* pts, int n);
  // Slam::AddFrames with one frame per LiDAR device (Slam.cxx:230-344, 753-801)
  struct InputFrame
  {
    const lsa_point_t* pts;
    int n;
    uint64_t stampUs;
    uint32_t seq;
  };
  int AddFrames(const InputFrame* frames, int nframes);
  // Slam::SetKeyPointsExtractor(extractor, deviceId) / SetBaseToLidarOffset(transform, deviceId) (Slam.h:239-250):
  // device 0 always has an extractor (ExtractParams); the others get one with their first parameter
  int SetExtractorParam(int deviceId, const std::string& name, double v);
  int GetExtractorParam(int deviceId, const std::string& name, double* v) const;
  int SetBaseToLidarOffset(int deviceId, const Pose& offset);
  Pose GetBaseToLidarOffset(int deviceId) const;

  Pose GetWorldTransform(double* time = nullptr) const;
  // Slam::GetLatencyCompensatedWorldTransform (Slam.cxx:555-590): the last pose extrapolated by Latency
  Pose GetLatencyCompensatedWorldTransform(double* time = nullptr) const;
  // Slam::SetWorldTransformFromGuess (Slam.cxx:490-501)
  int SetWorldTransformFromGuess(const Pose& guess);
  // Slam::GetDebugInformation (Slam.cxx:610-633): matches used by the last ego-motion / localization iteration per
  // type, registration errors, overlap, motion-limit compliance.  Reads five 32-byte histograms back on demand.
  int GetDebugInformation(double out[10]);
  const std::array<double, 36>& GetTransformCovariance() const { return LocalizationUncertainty.Covariance; }
  int GetKeypoints(int type, bool world, std::vector<lsa_point_t>& out);
  int GetRawKeypoints(int type, std::vector<lsa_point_t>& out);
  int GetRegisteredFrame(std::vector<lsa_point_t>& out);
  const MatchDebug& GetMatchDebug(bool localization, int type) const { return localization ? LocDebug[type] : EgoDebug[type]; }

  int SetParam(const std::string& name, double v);
  int GetParam(const std::string& name, double* v) const;
  // Slam::AddWheelOdomMeasurement / AddGravityMeasurement / ClearSensorMeasurements (Slam.cxx:1582-1598); the weights and
  // the time offset are the parameters WheelOdomWeight, GravityWeight, SensorTimeOffset.  Slam::Reset leaves them alone.
  SensorConstraints& Sensors() { return SensorManagers; }
  // the terms the last frame's localization solved with
  const lsa_sensor_terms_t& LocalizationSensorTerms() const { return LocSensorTerms; }
  // LocalMaps[k] after every pending insertion has landed (Slam::GetMap reads through this)
  RollingGrid& Map(int k) { WaitMaps(); return *LocalMaps[k]; }

  // ---- parameters (names = the reference's members) ----
  bool UseKeypoints[3] = {true, true, false};
  EgoMotionMode EgoMotion = EgoMotionMode::MOTION_EXTRAPOLATION;
  UndistortionMode Undistortion = UNDISTORTION_REFINED;
  bool TwoDMode = false;
  unsigned EgoMotionICPMaxIter = 4, LocalizationICPMaxIter = 3;
  unsigned EgoMotionLMMaxIter = 15, LocalizationLMMaxIter = 15;
  double EgoMotionMaxNeighborsDistance = 5., LocalizationMaxNeighborsDistance = 5.;
  unsigned EgoMotionEdgeNbNeighbors = 8, EgoMotionEdgeMinNbNeighbors = 3;
  double EgoMotionEdgeMaxModelError = 0.2;
  unsigned LocalizationEdgeNbNeighbors = 10, LocalizationEdgeMinNbNeighbors = 4;
  double LocalizationEdgeMaxModelError = 0.2;
  unsigned EgoMotionPlaneNbNeighbors = 5;
  double EgoMotionPlanarityThreshold = 0.04, EgoMotionPlaneMaxModelError = 0.2;
  unsigned LocalizationPlaneNbNeighbors = 5;
  double LocalizationPlanarityThreshold = 0.04, LocalizationPlaneMaxModelError = 0.2;
  unsigned LocalizationBlobNbNeighbors = 10;
  double EgoMotionInitSaturationDistance = 5., EgoMotionFinalSaturationDistance = 1.;
  double LocalizationInitSaturationDistance = 2., LocalizationFinalSaturationDistance = 0.5;
  double MaxExtrapolationRatio = 3.;
  unsigned MinNbMatchedKeypoints = 20;
  double KfDistanceThreshold = 0.5, KfAngleThreshold = 5.;
  MappingMode MapUpdate = MappingMode::UPDATE;
  // Confidence estimator: share of the frame's points with a map point nearby (Slam::SetOverlapSamplingRatio,
  // GetOverlapEstimation; 0 = off, the library default; the ROS configuration uses 0.33)
  float OverlapSamplingRatio = 0.f;
  float OverlapEstimation = -1.f;
  // Confidence estimator: velocity / acceleration over a time window against limits (Slam::CheckMotionLimits,
  // Slam.cxx:1391-1484; linear [m/s, m/s2] and angular [deg/s, deg/s2]); TimeWindowDuration = 0 turns it off
  float VelocityLimits[2] = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max()};
  float AccelerationLimits[2] = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max()};
  float TimeWindowDuration = 0.f;
  bool ComplyMotionLimits = true;
  // Slam::LoggingTimeout (Slam.h:425-438): 0 keeps the last two poses, > 0 the poses of that many seconds, < 0 all
  double LoggingTimeout = 0.;
  // Slam::LoggingStorage (Slam.h:440-447): accepted and remembered; the keypoint log is uncompressed in HBM whatever it says
  int LoggingStorage = 0;
  double Latency = 0.;  // duration of the last AddFrame [s] (Slam::GetLatency)
  Pose BaseToLidarOffset = Pose::Identity();  // device 0
  lsa_extract_params_t ExtractParams;         // device 0
  struct DeviceExtractor
  {
    lsa_extract_params_t params;
    float azimuthalResolution = 0.f;  // estimated from that device's first frame
  };
  std::map<int, DeviceExtractor> OtherExtractors;  // devices != 0
  std::map<int, Pose> OtherBaseToLidarOffsets;
  // edge length of the finest kNN search-grid cells (an implementation knob: results do not depend on it)
  double KnnCellSizeEgoMotion = 0.25;      // [m] previous-scan plane targets (dense)
  double KnnCellSizeEgoMotionEdges = 0.5;  // [m] previous-scan edge targets (sparse)
  double KnnCellScaleMaps = 1.0;           // x map leaf size, plane / blob sub-maps
  double KnnCellScaleMapsEdges = 2.5;      // x map leaf size, edge sub-maps
  // lanes per query in the first kNN kernel (sparse edge targets: more lanes, fewer queries per wavefront)
  int KnnLanesEdges = 16, KnnLanesPlanes = 8, KnnLanesBlobs = 8;
  int KnnRoundsEdges = 2, KnnRoundsPlanes = 2, KnnRoundsBlobs = 2;  // rounds of the first kNN kernel (2 or 3)
  // build the next frame's ego-motion targets beside this frame's registration (a scheduling knob: same results)
  bool BuildTargetsAhead = true;
  // LocalOptimizer::Solve as one launch (the trust-region loop on the device) instead of one launch per evaluation
  bool DeviceLM = true;
  // one ICP iteration's matching step as one launch (search + model fit fused, all types) instead of staged kernels
  bool FusedMatch = true;
  bool KeepMatchDebug = false;  // download MatchingResults::Rejections/Weights every frame (Slam::GetDebugArray)

  std::shared_ptr<RollingGrid> LocalMaps[3];
  // The same three maps resident on the device (lsa_device_grid: SURVEY.md 8f-1).  "MapsOnDevice" (default): keyframes
  // are inserted and sub-maps extracted without leaving the device -- no staging of the keypoints in host memory, no map
  // threads, no sub-map upload.  Off: the host containers above.  Both
  // hand their points out in the same order ("OrderedMaps": 1 key order, 0 the reference's container order), so the two
  // give the same sub-maps and the same poses.
  lsa_device_grid* DevMaps[3] = {nullptr, nullptr, nullptr};
  bool MapsOnDevice = true;
  // device maps: sub-maps extracted for the predicted boxes beside the ego-motion ICP ("SubMapsAhead"): the extraction and
  // the spare target's search grid queue on the look-ahead stream behind the previous keyframe's insertions, a host thread
  // of their own enqueues them, and the localization swaps the target in when the actual box touches the same outer voxels
  // (980 against 950 frames/s; with the first, slower insertion kernels it lost: the sub-map came 0.05 ms late)
  bool SubMapsAhead = true;
  bool SubMapsAheadAdaptive = true;  // give it up for a while when the localization had to wait for it twice in a row
  bool LocalizationStartFused = true;  // reset + first undistortion + keypoint boxes of the localization as one launch (device maps)
  int ICPAhead = 2;               // ICP iterations enqueued ahead of their inputs.  0: off (in line); anything else: the whole loop at once, every solve leaving the next iteration's pose on the device (lsa_icp_link).  1 once selected another schedule and stays accepted as a synonym of 2
  bool UndistortInSearch = true;  // RefineUndistortion between two localization iterations inside the next iteration's search kernel
  bool SpecBoxesOnLookahead = true;  // the predicted boxes of the sub-maps ahead of time on the look-ahead stream, not the context's
  bool SpecGridsTogether = true;  // the search grids of the sub-maps extracted ahead of time built by one sequence of launches
  bool DevSpec[3] = {false, false, false};
  bool OrderedMaps = true;
  bool DeviceMapsInUse() const { return MapsOnDevice && DevMaps[0]; }  // (every sampling mode: CENTROID since round 3)
  int MigrateMaps(bool fromDevice);
  int SetParamValue(const std::string& name, double v);
  int GetMap(int k, bool clean, std::vector<lsa_point_t>& out);
  int GetTargetSubMap(int k, std::vector<lsa_point_t>& out);

  // ---- the dense point-cloud map (lsa_slam_dense.cpp; lsa_dense_*.hip) ----
  // "DenseMap": 0 off (nothing whatever changes), 1 every registered frame, 2 keyframes only.  The frame or frames of an
  // AddFrame(s) call go into a voxel hash table on the device at its end, under the poses GetRegisteredFrame would use, all
  // with one ordinal: the count of inserted calls.  Cleared by Reset, ClearMaps and every applied trajectory (the points
  // were placed under the old poses).  The four calls wait for the insertions in flight and refuse while the map is off.
  int DenseMapMode = 0;
  double DenseMapLeafSize = 0.1;
  double DenseMapMaxBytes = 16. * 1024. * 1024. * 1024.;  // of the table; 0: no limit
  double DenseMapGridMaxCells = 16777216.;  // the map's "GridMaxCells": the most cells GetDenseMapGrid hands out
  unsigned DenseFrames = 0, DenseRefused = 0, DenseClears = 0;
  // "DenseMapOnTrajectory": what an applied trajectory does to the map.  0 clears it (the default); 1 re-projects it on the
  // device, every voxel's point under new * inverse(old) of the logged pose of the frame that measured it
  // (ReprojectDenseMap), and the ordinals go on.  Reset, ClearMaps and ClearDenseMap clear under either value.
  int DenseMapOnTrajectory = 0;
  unsigned DenseReprojections = 0;
  int DenseMapSize();
  int GetDenseMap(int minFrames, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity);
  int GetDenseMapSources(int minFrames, int* out, int capacity);
  int SaveDenseMapToPCD(const std::string& path, int format, int minFrames);
  int ClearDenseMap();
  // free space: "DenseMapCarve" 0 off (the default: one more untaken branch), 1 the rays of every inserted
  // frame are walked once all device frames of the call are in the map; the three knobs are lsa_dense_map_set's
  int DenseMapCarve = 0;
  double DenseMapCarveRange = 30., DenseMapCarveMarginLeaves = 2., DenseMapCarveStride = 1.;
  int GetDenseMapFiltered(int minFrames, double maxMissRatio, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity);
  int GetDenseMapMisses(int minFrames, double maxMissRatio, uint32_t* out, int capacity);
  int SaveDenseMapToPCDFiltered(const std::string& path, int format, int minFrames, double maxMissRatio);
  int PruneDenseMap(int minFrames, double maxMissRatio, long long* removed);
  int GetRegisteredFrameOrigins(std::vector<float>& out);
  // normals: computed from the table as it stands, towards the viewpoints below when `orient`
  int GetDenseMapNormals(int minFrames, double maxMissRatio, int radiusLeaves, int minNeighbors, int orient, lsa_dense_normal_t* out, int capacity);
  int SaveDenseMapToPCDNormals(const std::string& path, int format, int minFrames, double maxMissRatio, int radiusLeaves, int minNeighbors, int orient);
  int GetDenseMapViewpoints(float* xyz, int capacity, int* firstFrame);
  // the floor plan: elevation, ground and the occupancy grid, rasterised from the table as it stands
  long long GetDenseMapGrid(const lsa_dense_grid_params_t* params, lsa_dense_grid_info_t* info, lsa_dense_cell_t* cells, int8_t* state, long long capacity);
  long long SaveDenseMapGrid(const lsa_dense_grid_params_t* params, const std::string& prefix);
  // rays (DESIGN.md 3.14 "Rays"; lsa_dense_cast.hip): questions along a line, answered from the table as it stands; nothing is
  // added to a frame.  DenseLastOrdinal: the ordinal under which the call that brought the current frame went into the map, -1
  // when it did not (mode 2 and no keyframe, a refused insertion, a frame that failed or came while "DenseMap" was 0, a cleared
  // map): reset where the current frame changes (ProcessCurrentFrame); what use_before == 2 of the compare resolves to
  int DenseLastOrdinal = -1;
  int CastDenseMapRays(const float* origins, int nOrigins, const float* targets, int n, const lsa_dense_cast_params_t* params, lsa_dense_hit_t* hits, lsa_point_t* points);
  int RenderDenseMapScan(const double* pose16, const double* elevations, int nRings, int nAzimuth, const lsa_dense_cast_params_t* params, lsa_dense_hit_t* hits);
  int CompareFrameToDenseMap(const lsa_dense_cast_params_t* params, uint8_t* labels, int capacity, long long counts[4]);

  // ---- state ----
  Pose Tworld, PreviousTworld, Trelative;
  RegistrationError LocalizationUncertainty;
  unsigned TotalMatchedKeypoints = 0;
  unsigned NbrFrameProcessed = 0;
  unsigned SubMapSpecHitsTotal = 0;
  int KfCounter = 0;
  FrameStats Stats;
  std::deque<StampedPose> LogTrajectory;
  std::deque<std::array<double, 36>> LogCovariances;
  int KeypointCounts[3] = {0, 0, 0};

private:
  int Fail(int rc, const char* where);
  // what the context's table of map descriptors was made of when the maps live on the host: the device grids keep count themselves
  struct HostMapTable
  {
    bool valid = false;
    lsa_place_params_t params;
    std::vector<double> viewpoints;
    unsigned long long modifications[3] = {0, 0, 0};
  } MapPlaceHostTable;
  lsa_ctx* Ctx = nullptr;
  std::string LastError;

  // ---- frame path (lsa_slam_core.cpp) ----
  int ProcessCurrentFrame(uint64_t stampUs);
  int ExtractKeypoints();
  int ExtractFrames();
  int PrepareNextEgoMotionTargets();
  int EstimateOverlap();
  void CheckMotionLimits();
  unsigned UsedTypesMask() const { return (UseKeypoints[0] ? 1u : 0u) | (UseKeypoints[1] ? 2u : 0u) | (UseKeypoints[2] ? 4u : 0u); }  // bit k: type k is in use
  void ApplySearchTuning(lsa_ctx* ctx);  // the search's form and tuning (results do not depend on either)
  // the frames of the current AddFrames call when there are several (device-resident, in the last slots of the
  // context's frame store); empty for the single-frame calls, whose frame is the context's current one
  struct HeldFrame
  {
    int slot;
    int n;
    int device;
    double timeOffset;  // stamp - first frame's stamp [s]
  };
  std::vector<HeldFrame> CurrentFrames;
  float Device0AzimuthalResolution = 0.f;  // parked here while another device's frame is extracted
  uint64_t CurrentStamp = 0;
  bool HaveFrame = false;
  double CurrentTime = 0.;
  Pose KfLastPose;
  float PreviousVelocity[2] = {0.f, 0.f};
  std::vector<lsa_point_t> Scratch;
  SensorConstraints SensorManagers;
  lsa_sensor_terms_t LocSensorTerms = {};

  // ---- ICP loops and undistortion (lsa_slam_icp.cpp; the loop is lsa_slam_icp_loop.h) ----
  int ComputeEgoMotion();
  int Localization();
  // The ICP loop of both, and of RegisterLoggedFrames, under whichever schedule ICPAhead allows: the spec says what the loop
  // matches and solves, the callables what only one of them does at that point of an iteration.
  struct IcpLoopSpec;
  struct IcpUndistortion;
  template <class Top, class Enqueued, class Solved, class Skipped, class Accepted, class Finished>
  int RunIcpLoop(const IcpLoopSpec& spec, Pose& pose, const Top& top, const Enqueued& enqueued, const Solved& solved, const Skipped& skipped,
                 const Accepted& accepted, const Finished& finished);
  lsa_match_params_t EgoMatchParams() const;
  lsa_match_params_t LocMatchParams() const;
  int DownloadMatchDebug(int set, unsigned typeMask, MatchDebug* debug);
  Pose InterpolateScanPose(double time) const;
  int InitUndistortion();
  void InitUndistortion(double t0, double t1);
  int RefineUndistortion(Pose* outD0 = nullptr, Pose* outD1 = nullptr);
  WithinFrameMotion Motion;
  long long EgoMatchSerial[3] = {0, 0, 0}, LocMatchSerial[3] = {0, 0, 0};  // lsa_match_serial after the last iteration
  MatchDebug EgoDebug[3], LocDebug[3];

  // ---- sub-maps and speculation (lsa_slam_maps.cpp) ----
  // What Localization() searches: which sub-maps are stale, what the speculation left is taken or dropped, the rest extracted
  int PrepareLocalizationSubMaps(bool boxesEnqueued);
  int UpdateMapsUsingTworld();
  // edge length of the search cells of map k's target: the map holds one point per leaf voxel, a cell of about one leaf keeps a handful of candidates
  float MapSearchCell(int k) const { return static_cast<float>((k == LSA_EDGE ? KnnCellScaleMapsEdges : KnnCellScaleMaps) * LocalMaps[k]->GetLeafSize()); }
  // Sub-maps are extracted ahead of time: as soon as the keypoints exist, their bounding box under the
  // PREDICTED pose is reduced on the device (asynchronously) and the map workers extract the sub-maps for it
  // while the ego-motion ICP runs.  Localization() checks the box under the actual pose: the sub-map only
  // depends on the range of 10 m voxels the box touches, which a pose refinement rarely changes; if it did,
  // the sub-map is extracted again.  Same result either way.
  int BeginSubMapSpeculation(const Pose& predicted);
  int FinishSubMapSpeculation();
  int StageSpeculativeSubMaps();
  void DropMapLookahead();  // sub-maps extracted ahead and spare targets made from the maps as they were
  bool SpecPending = false;
  bool SpecBuilt[3] = {false, false, false};  // written by the workers, read after WaitMaps
  // the same news for the thread that runs the ICP: it hands a finished sub-map to the device (upload and search
  // grid on the look-ahead stream) at its next stop between two kernels' results
  std::atomic<bool> SpecDone[3];
  bool SpecStaged[3] = {false, false, false};
  // ... with the maps on the device (DevSpec[k] above: a sub-map of map k was asked for ahead of time)
  int DevSpecStatus = 0;   // written by the look-ahead thread, read once DevSpecRunning is false
  std::atomic<bool> DevSpecRunning{false};
  int DevSpecBackoff = 0;  // frames the sub-maps ahead of time are not tried for (they were late)
  int DevSpecLate = 0;     // frames in a row the localization had to wait for them
  int DevSpecGood = 0, DevSpecPenalty = 4;
  double MapJobSeconds[3] = {0., 0., 0.};  // written by the workers, read after WaitMaps
  int MapJobFailed[3] = {0, 0, 0};         // a device-map insertion that failed on its worker (read after WaitMaps)

  // ---- look-ahead and interlude (lsa_slam_core.cpp) ----
  int TryStartLookahead();        // starts the announced cloud's extraction as soon as its upload has been enqueued
  void ArmLookaheadInterlude();
  int InterludeWork();
  int FinishLookaheadInterlude();
  bool InterludeRan = true;
  int InterludeStatus = 0;
  int NextStoredSlot = -1;
  bool NextFrameHinted = false;   // a cloud was announced (HintNextFrame) and its look-ahead extraction not started yet
  bool HoldLookahead = false;     // ... and must not start yet: the sub-maps extracted ahead of time for THIS frame's localization go onto the look-ahead stream first
  int AheadStatus = 0;            // result of the work the look-ahead thread did beside the first ego-motion solve

  // ---- keypoint log and the scratch context (lsa_slam_log.cpp) ----
  void LogCurrentFrameState(double time);
  bool KpLogStopped = false;  // a chunk of the keypoint log could not be allocated: nothing more is logged until Reset(true)
  // What every call on the log refuses first: logging off (`whatIsMissing` ends that sentence), logging stopped and, with
  // `covering`, LogCovers.  Returns the number of logged poses, or the refusal's code with its text in LastError.
  int LogReady(const std::string& who, const char* whatIsMissing, bool covering = true);
  int LogCovers(const std::string& who);  // refuses a keypoint log that has fewer frames than there are logged poses
  void LoggedPoses16(std::vector<double>& poses, std::vector<double>* times) const;  // the logged trajectory, 16 doubles a pose
  std::vector<double> RowsOf(const double* poses16, int n) const;  // rows of lsa_slam_get_trajectory: the poses dated like the log
  // the two pose-graph calls: what both refuse and pack before their own part, and everything from the solve on
  struct PoseGraphProblem;
  int PoseGraphBegin(const std::string& who, const lsa_pgo_params_t* params, const std::string& tooFew, int capacity, PoseGraphProblem& pb);
  int PoseGraphEdges(const std::string& who, const lsa_pgo_edge_t* loopEdges, int m, PoseGraphProblem& pb);
  template <class Solve>
  int PoseGraphSolve(const std::string& who, const PoseGraphProblem& pb, const Solve& solve, double* poses17, lsa_pgo_result_t* result);
  int LoggedChainEdges(const lsa_pgo_params_t& p, const std::string& who, lsa_pgo_edge_t* edges);
  // RegisterLoggedFrames' and the pose-graph solves' own context on the same device, made by the first call: the query
  // keypoints (its working set), a scratch map per keypoint type and the targets their sub-maps become
  lsa_ctx* LoopCtx = nullptr;
  lsa_device_grid* LoopMaps[3] = {nullptr, nullptr, nullptr};
  int EnsureLoopClosureScratch();

  // ---- the dense map (lsa_slam_dense.cpp) ----
  lsa_dense_map* Dense = nullptr;  // made by the first insertion
  bool DenseWarned = false;
  std::vector<double> DenseTimes;  // per ordinal, the time under which LogCurrentFrameState logged the frame
  std::vector<float> DenseViewpoints;  // per ordinal, xyz: where the call's first sensor stood (12 B a frame); entry 0 is ordinal 0
  int InsertDenseFrame(bool keyframe, double time);
  // the corrections of the dense ordinals still logged (from *firstOrdinal on) for the trajectory poses16 about to replace
  // the logged one; false when the map is to be cleared instead
  bool DenseCorrections(const double* poses16, int n, std::vector<double>& corrections, int* firstOrdinal) const;
  int ReprojectDenseMap(const std::vector<double>& corrections, int firstOrdinal);
  void DropDenseMap(const char* why);  // why == nullptr: the caller asked for it, nothing to warn about
  int DenseReady(const char* who);
  int MakeDenseMap();  // the map with the pipeline's knobs, when there is none yet
  int SetDenseCarveParams();  // the knobs into the map, when there is one

  // ---- diagnostics ----
  double DbgAcc[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // (LSA_STAGE_DEBUG=1: seconds outside the stage timers, printed when the object goes)
  long DbgFrames = 0;
  double PoseGraphSeconds = 0.;   // the last OptimizeLoggedTrajectory's or RunPoseGraphOptimization's solve by the host's clock
  double LoopClosureSeconds[4] = {0., 0., 0., 0.};  // the last call by the host's clock: replays, scratch maps, ICP loop, all of it

  // ---- workers ----
  // These stay the LAST data members: members are destroyed in reverse order of declaration, so the threads are joined
  // before any state their jobs touch goes away (and they start after all of it exists).
  bool WorkerPrewake = true;  // the worker threads are woken ahead of the jobs whose time is known (HostWorker::Expect)
  void WaitMaps() { for (auto& w : MapWorker) w.Wait(); AheadWorker.Wait(); }
  HostWorker AheadWorker;     // enqueues the sub-maps ahead of time and the next frame's ego-motion targets beside the first solve
  HostWorker MapWorker[3];    // one per map: the three rolling grids are independent
};

}  // namespace host
}  // namespace lsa
