// lsa_slam_params.cpp -- SlamCore's parameters by name: the table, the setters that do more than assign, the extractors
// and offsets of the other LiDAR devices.
#include "lsa_slam_internal.h"
#include <algorithm>

namespace lsa
{
namespace host
{
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
  if (name == "DenseMap")
  {
    if (!(v == 0. || v == 1. || v == 2.)) { LastError = "DenseMap: 0 off, 1 every registered frame, 2 keyframes only"; return LSA_E_ARG; }
    DenseMapMode = static_cast<int>(v);
    return LSA_OK;
  }
  if (name == "DenseMapLeafSize")
  {
    if (!(v > 0.) || !(v < 1e9)) { LastError = "DenseMapLeafSize: a positive length"; return LSA_E_ARG; }
    // the voxels of a map made under another leaf size mean nothing under this one: the next insertion makes a new map
    if (Dense && v != DenseMapLeafSize) { lsa_dense_map_destroy(Dense); Dense = nullptr; DenseFrames = 0; DenseTimes.clear(); DenseViewpoints.clear(); }
    DenseMapLeafSize = v;
    return LSA_OK;
  }
  if (name == "DenseMapMaxBytes")
  {
    if (!(v >= 0.)) { LastError = "DenseMapMaxBytes: >= 0 (0: no limit)"; return LSA_E_ARG; }
    DenseMapMaxBytes = v;
    if (Dense) lsa_dense_map_set(Dense, "MaxBytes", v);
    return LSA_OK;
  }
  if (name == "DenseMapGridMaxCells")
  {
    if (!(v >= 1.) || v > 268435456. || v != static_cast<double>(static_cast<long long>(v))) { LastError = "DenseMapGridMaxCells: a whole number between 1 and 2^28"; return LSA_E_ARG; }
    DenseMapGridMaxCells = v;
    if (Dense) lsa_dense_map_set(Dense, "GridMaxCells", v);
    return LSA_OK;
  }
  if (name == "DenseMapCarve")
  {
    if (!(v == 0. || v == 1.)) { LastError = "DenseMapCarve: 0 off, 1 the rays of every inserted frame carve free space"; return LSA_E_ARG; }
    DenseMapCarve = static_cast<int>(v);
    return DenseMapCarve ? SetDenseCarveParams() : LSA_OK;
  }
  if (name == "DenseMapCarveRange" || name == "DenseMapCarveMarginLeaves" || name == "DenseMapCarveStride")
  {
    double& knob = name == "DenseMapCarveRange" ? DenseMapCarveRange : (name == "DenseMapCarveMarginLeaves" ? DenseMapCarveMarginLeaves : DenseMapCarveStride);
    const bool ok = name == "DenseMapCarveRange" ? (v > 0. && v / DenseMapLeafSize <= 4096.)
                    : name == "DenseMapCarveMarginLeaves" ? (v >= 0. && v < 1e9) : (v >= 1. && v <= 1e9 && v == static_cast<double>(static_cast<long long>(v)));
    if (!ok) { LastError = name + ": out of range (a range of at most 4096 leaves, a margin >= 0, a whole stride >= 1)"; return LSA_E_ARG; }
    knob = v;
    return SetDenseCarveParams();
  }
  if (name == "DenseMapOnTrajectory")
  {
    if (!(v == 0. || v == 1.)) { LastError = "DenseMapOnTrajectory: 0 an applied trajectory clears the dense map, 1 it re-projects it"; return LSA_E_ARG; }
    DenseMapOnTrajectory = static_cast<int>(v);
    return LSA_OK;
  }
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
  if (name == "DenseMap") { *v = DenseMapMode; return LSA_OK; }
  if (name == "DenseMapLeafSize") { *v = DenseMapLeafSize; return LSA_OK; }
  if (name == "DenseMapMaxBytes") { *v = DenseMapMaxBytes; return LSA_OK; }
  if (name == "DenseMapGridMaxCells") { *v = DenseMapGridMaxCells; return LSA_OK; }
  if (name == "DenseMapCapacity") { *v = Dense ? lsa_dense_map_get_param(Dense, "Capacity") : 0.; return LSA_OK; }
  // (the two that count on the device wait for the insertions in flight)
  if (name == "DenseMapVoxels") { *v = Dense ? std::max(lsa_dense_map_size(Dense), 0) : 0; return LSA_OK; }
  if (name == "DenseMapSkipped") { *v = Dense ? static_cast<double>(std::max(lsa_dense_map_skipped(Dense), 0ll)) : 0.; return LSA_OK; }
  if (name == "DenseMapBytes") { *v = Dense ? static_cast<double>(lsa_dense_map_bytes(Dense)) : 0.; return LSA_OK; }
  if (name == "DenseMapRefusedFrames") { *v = DenseRefused; return LSA_OK; }
  if (name == "DenseMapClears") { *v = DenseClears; return LSA_OK; }
  if (name == "DenseMapFrames") { *v = DenseFrames; return LSA_OK; }
  if (name == "DenseMapOnTrajectory") { *v = DenseMapOnTrajectory; return LSA_OK; }
  if (name == "DenseMapCarve") { *v = DenseMapCarve; return LSA_OK; }
  if (name == "DenseMapCarveRange") { *v = DenseMapCarveRange; return LSA_OK; }
  if (name == "DenseMapCarveMarginLeaves") { *v = DenseMapCarveMarginLeaves; return LSA_OK; }
  if (name == "DenseMapCarveStride") { *v = DenseMapCarveStride; return LSA_OK; }
  if (name == "DenseMapRays") { *v = Dense ? std::max(lsa_dense_map_get_param(Dense, "Rays"), 0.) : 0.; return LSA_OK; }
  if (name == "DenseMapPruned") { *v = Dense ? lsa_dense_map_get_param(Dense, "Pruned") : 0.; return LSA_OK; }
  if (name == "DenseMapReprojections") { *v = DenseReprojections; return LSA_OK; }
  if (name == "DenseMapDropped") { *v = Dense ? lsa_dense_map_get_param(Dense, "Dropped") : 0.; return LSA_OK; }
  if (name == "DenseMapReprojectSeconds") { *v = Dense ? lsa_dense_map_get_param(Dense, "ReprojectSeconds") : 0.; return LSA_OK; }
  if (name == "DenseMapRehashes") { *v = Dense ? lsa_dense_map_get_param(Dense, "Rehashes") : 0.; return LSA_OK; }
  if (name == "DenseMapExportSeconds") { *v = Dense ? lsa_dense_map_get_param(Dense, "ExportSeconds") : 0.; return LSA_OK; }
  return LSA_E_ARG;
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

}  // namespace host
}  // namespace lsa
