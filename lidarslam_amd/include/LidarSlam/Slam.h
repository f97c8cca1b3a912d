// LidarSlam/Slam.h -- source-level mirror of the reference's public C++ API on top of the C ABI.
//
// Same namespace, class and method names as slam_lib/include/LidarSlam/Slam.h:98-394 for the part of
// the API that drives the per-frame hot path, so that a caller written against the reference
// (ros_wrapping/lidar_slam/src/LidarSlamNode.cxx:173, paraview_wrapping/.../vtkSlam.cxx:217) compiles
// against this header and links liblidarslam_amd.so instead of libLidarSlam.  Header only: every
// method forwards to include/lidarslam_amd.h.
//
// PCL / Eigen: when <pcl/point_cloud.h> is available the real pcl::PointCloud is used; otherwise a
// minimal shim with the members the reference touches (points, header{stamp,frame_id,seq}, size, empty,
// push_back, front, back, reserve, clear, Ptr) is provided so that this header is usable in images
// without PCL (such as the build container).  Poses are exchanged as row-major 4x4 doubles; with Eigen
// present Transform::GetIsometry() is offered as well.
//
// Beyond the per-frame path the mirror also carries PCD map IO, the wheel odometer / IMU gravity constraints, the keypoint
// log (SetLoggingTimeout, SetLoggingStorage, GetLoggedKeypoints) and SetTrajectoryAndRebuildMaps, which brings a corrected
// trajectory back, and the loop-closure constraint an optimizer needs as input: FindLoopClosureCandidate and
// RegisterLoggedFrames.  OptimizeLoggedTrajectory optimizes the logged trajectory with such edges on the device, and
// RunPoseGraphOptimization, the reference's entry point with GPS positions, runs on the same device solver with the positions
// as priors (no g2o).  Both have an overload that takes RobustParameters -- a robust loss on the loop edges or on the GPS priors --
// and gives a ConstraintVerdict {chi2, weight} per constraint, so that a false loop edge or an outlying fix is discounted and seen.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include "lidarslam_amd.h"

#include "Enums.h"
#include "LidarPoint.h"
#include "SpinningSensorKeypointExtractor.h"

namespace LidarSlam
{

// slam_lib/include/LidarSlam/Transform.h:25-79.  The pose is kept as a row-major 4x4 (what the C ABI speaks); with
// Eigen present (LSA_HAVE_EIGEN) the reference's Eigen constructors and accessors are offered with their own types.
struct Transform
{
  std::array<double, 16> matrix{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};  // row-major
  double time = 0.;
  std::string frameid;

  Transform() = default;
  // Euler angles ZYX convention (R = Rz(rz) Ry(ry) Rx(rx)), as Utils::XYZRPYtoIsometry (slam_lib/src/Utilities.cxx:62-69)
  Transform(double x, double y, double z, double rx, double ry, double rz, double t = 0., const std::string& frame = "") : time(t), frameid(frame)
  {
    const double cx = std::cos(rx), sx = std::sin(rx), cy = std::cos(ry), sy = std::sin(ry), cz = std::cos(rz), sz = std::sin(rz);
    matrix = {{cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz, x,
               cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz, y,
               -sy, sx * cy, cx * cy, z,
               0, 0, 0, 1}};
  }
  explicit Transform(const std::array<double, 16>& rowMajor, double t = 0., const std::string& frame = "") : matrix(rowMajor), time(t), frameid(frame) {}
  static Transform Identity() { return Transform(); }

  double& x() { return matrix[3]; }
  double& y() { return matrix[7]; }
  double& z() { return matrix[11]; }
  double x() const { return matrix[3]; }
  double y() const { return matrix[7]; }
  double z() const { return matrix[11]; }
  const std::array<double, 16>& GetMatrixArray() const { return matrix; }
#ifdef LSA_HAVE_EIGEN
  Transform(const Eigen::Matrix<double, 6, 1>& xyzrpy, double t = 0., const std::string& frame = "")
    : Transform(xyzrpy(0), xyzrpy(1), xyzrpy(2), xyzrpy(3), xyzrpy(4), xyzrpy(5), t, frame) {}
  Transform(const Eigen::Vector3d& trans, const Eigen::Vector3d& rpy, double t = 0., const std::string& frame = "")
    : Transform(trans(0), trans(1), trans(2), rpy(0), rpy(1), rpy(2), t, frame) {}
  Transform(const Eigen::Isometry3d& transform, double t = 0., const std::string& frame = "") : time(t), frameid(frame) { this->SetIsometry(transform); }
  Transform(const Eigen::Translation3d& trans, const Eigen::Quaterniond& rot, double t = 0., const std::string& frame = "") : time(t), frameid(frame)
  {
    this->SetIsometry(Eigen::Isometry3d(trans * rot.normalized()));
  }
  void SetIsometry(const Eigen::Isometry3d& isometry)
  {
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) matrix[r * 4 + c] = isometry.matrix()(r, c);
  }
  Eigen::Isometry3d GetIsometry() const
  {
    Eigen::Isometry3d iso = Eigen::Isometry3d::Identity();
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) iso(r, c) = matrix[r * 4 + c];
    return iso;
  }
  Eigen::Vector3d GetPosition() const { return Eigen::Vector3d(matrix[3], matrix[7], matrix[11]); }
  Eigen::Translation3d GetTranslation() const { return Eigen::Translation3d(this->GetPosition()); }
  Eigen::Quaterniond GetRotation() const { return Eigen::Quaterniond(this->GetIsometry().linear()); }
  Eigen::Matrix4d GetMatrix() const { return this->GetIsometry().matrix(); }
#else
  // without Eigen: position as an array, the matrix as the row-major array
  std::array<double, 3> GetPosition() const { return {{matrix[3], matrix[7], matrix[11]}}; }
  const std::array<double, 16>& GetMatrix() const { return matrix; }
#endif
};

// slam_lib/include/LidarSlam/PointCloudStorage.h:60-75 (the values callers pass to SaveMapsToPCD / SetLoggingStorage)
enum PCDFormat { ASCII = 0, BINARY = 1, BINARY_COMPRESSED = 2 };
enum PointCloudStorageType { PCL_CLOUD = 0, OCTREE_COMPRESSED = 1, PCD_ASCII = 2, PCD_BINARY = 3, PCD_BINARY_COMPRESSED = 4 };

// slam_lib/include/LidarSlam/SensorConstraints.h:13-23 (external sensors: constraints of the localization solve -- see the Slam methods)
namespace SensorConstraints
{
struct WheelOdomMeasurement
{
  double Time = 0.;
  double Distance = 0.;
};
struct GravityMeasurement
{
  double Time = 0.;
#ifdef LSA_HAVE_EIGEN
  Eigen::Vector3d Acceleration = Eigen::Vector3d::Zero();
#else
  std::array<double, 3> Acceleration{{0., 0., 0.}};
#endif
};
}  // namespace SensorConstraints

#define LSA_SLAM_PARAM(name, type)                                                          \
  void Set##name(type v) { this->SetParam(#name, static_cast<double>(v)); }                 \
  type Get##name() const { return static_cast<type>(this->GetParam(#name)); }
#define LSA_SLAM_ENUM_PARAM(name, type)                                                     \
  void Set##name(type v) { this->SetParam(#name, static_cast<double>(static_cast<int>(v))); } \
  type Get##name() const { return static_cast<type>(static_cast<int>(this->GetParam(#name))); }

class Slam
{
public:
  using Point = LidarPoint;
  using PointCloud = pcl::PointCloud<Point>;

  // Throws when no HIP device is usable: the device path is the only path.
  explicit Slam(int device = 0)
  {
    if (lsa_slam_create(device, &this->Handle) != LSA_OK)
      throw std::runtime_error("LidarSlam::Slam: no usable HIP device (liblidarslam_amd has no CPU fallback)");
  }
  ~Slam() { lsa_slam_destroy(this->Handle); }
  Slam(const Slam&) = delete;
  Slam& operator=(const Slam&) = delete;

  void Reset(bool resetLog = true) { lsa_slam_reset(this->Handle, resetLog ? 1 : 0); }

  // ---- main use (Slam.h:111-146)
  void AddFrame(const PointCloud::Ptr& pc) { this->AddFrames({pc}); }
  // one frame per LiDAR device (at most 16): extracted with the device's extractor, merged in BASE (Slam.cxx:753-801)
  void AddFrames(const std::vector<PointCloud::Ptr>& frames)
  {
    if (frames.empty() || !frames[0]) return;
    if (frames.size() > 16)
    {
      this->LastError = "AddFrames: at most 16 frames (LiDAR devices) per call";
      std::fprintf(stderr, "\033[1;31m[ERROR] %s\033[0m\n", this->LastError.c_str());
      return;
    }
    const lsa_point_t* pts[16];
    int n[16];
    std::uint64_t stamps[16];
    std::uint32_t seqs[16];
    for (std::size_t i = 0; i < frames.size(); ++i)
    {
      const bool some = frames[i] && !frames[i]->empty();
      pts[i] = some ? reinterpret_cast<const lsa_point_t*>(frames[i]->points.data()) : nullptr;
      n[i] = some ? static_cast<int>(frames[i]->size()) : 0;
      stamps[i] = frames[i] ? frames[i]->header.stamp : frames[0]->header.stamp;
      seqs[i] = frames[i] ? frames[i]->header.seq : 0;
    }
    this->CurrentStamp = frames[0]->header.stamp;
    const int rc = lsa_slam_add_frames(this->Handle, pts, n, stamps, seqs, static_cast<int>(frames.size()));
    if (rc < 0) this->LastError = lsa_slam_last_error(this->Handle);  // like the reference: report, keep the previous pose
  }
  Transform GetWorldTransform() const
  {
    Transform t;
    lsa_slam_get_world_transform(this->Handle, t.matrix.data(), &t.time);
    t.frameid = this->WorldFrameId;
    return t;
  }
  // the last pose extrapolated by the duration of the last AddFrame (Slam.cxx:555-590)
  Transform GetLatencyCompensatedWorldTransform() const
  {
    Transform t;
    lsa_slam_get_latency_compensated_world_transform(this->Handle, t.matrix.data(), &t.time);
    t.frameid = this->WorldFrameId;
    return t;
  }
  std::array<double, 36> GetTransformCovariance() const
  {
    std::array<double, 36> c{};
    lsa_slam_get_covariance(this->Handle, c.data());
    return c;
  }
  // Slam.h:150-151; the log holds two poses unless SetLoggingTimeout was given something else than 0
  std::vector<Transform> GetTrajectory() const
  {
    const int n = lsa_slam_get_trajectory(this->Handle, nullptr, nullptr, 0);
    std::vector<double> rows(static_cast<std::size_t>(n > 0 ? n : 0) * 17);
    if (n > 0) lsa_slam_get_trajectory(this->Handle, rows.data(), nullptr, n);
    std::vector<Transform> poses(n > 0 ? n : 0);
    for (int i = 0; i < n; ++i)
    {
      std::memcpy(poses[i].matrix.data(), rows.data() + 17 * i, 16 * sizeof(double));
      poses[i].time = rows[17 * i + 16];
      poses[i].frameid = this->WorldFrameId;
    }
    return poses;
  }
  std::vector<std::array<double, 36>> GetCovariances() const
  {
    const int n = lsa_slam_get_trajectory(this->Handle, nullptr, nullptr, 0);
    std::vector<std::array<double, 36>> covs(n > 0 ? n : 0);
    if (n > 0) lsa_slam_get_trajectory(this->Handle, nullptr, covs[0].data(), n);
    return covs;
  }
  // Slam.h:155-158
  PointCloud::Ptr GetMap(Keypoint k, bool clean = false)
  {
    return this->Fetch([&](lsa_point_t* out, int cap) { return std::min(cap, lsa_slam_get_map(this->Handle, k, clean ? 1 : 0, out, cap)); }, this->WorldFrameId);
  }
  PointCloud::Ptr GetTargetSubMap(Keypoint k)
  {
    return this->Fetch([&](lsa_point_t* out, int cap) { return std::min(cap, lsa_slam_get_target_submap(this->Handle, k, out, cap)); }, this->WorldFrameId);
  }
  // Slam.h:189
  void SetWorldTransformFromGuess(const Transform& poseGuess) { lsa_slam_set_world_transform_from_guess(this->Handle, poseGuess.matrix.data()); }
  // Slam.h:176 (same keys)
  std::unordered_map<std::string, double> GetDebugInformation() const
  {
    double v[10] = {};
    lsa_slam_get_debug_information(this->Handle, v);
    return {{"EgoMotion: edges used", v[0]}, {"EgoMotion: planes used", v[1]}, {"Localization: edges used", v[2]},
            {"Localization: planes used", v[3]}, {"Localization: blobs used", v[4]}, {"Localization: position error", v[5]},
            {"Localization: orientation error", v[6]}, {"Confidence: overlap", v[7]}, {"Confidence: comply motion limits", v[8]}};
  }
  // worldCoordinates = false: BASE (undistorted), true: WORLD (Slam.cxx:690-702)
  PointCloud::Ptr GetKeypoints(Keypoint k, bool worldCoordinates = false)
  {
    return this->Fetch([&](lsa_point_t* out, int cap) { return lsa_slam_get_keypoints(this->Handle, k, worldCoordinates ? 1 : 0, out, cap); },
                       worldCoordinates ? this->WorldFrameId : this->BaseFrameId);
  }
  PointCloud::Ptr GetRegisteredFrame()
  {
    return this->Fetch([&](lsa_point_t* out, int cap) { return lsa_slam_get_registered_frame(this->Handle, out, cap); }, this->WorldFrameId);
  }
  unsigned int GetNbrFrameProcessed() const { return static_cast<unsigned int>(this->GetParam("NbrFrameProcessed")); }
  int GetTotalMatchedKeypoints() const { return static_cast<int>(this->GetParam("TotalMatchedKeypoints")); }
  // Confidence estimator (Slam.h: GetOverlapSamplingRatio / SetOverlapSamplingRatio / GetOverlapEstimation)
  float GetOverlapSamplingRatio() const { return static_cast<float>(this->GetParam("OverlapSamplingRatio")); }
  void SetOverlapSamplingRatio(float ratio) { this->SetParam("OverlapSamplingRatio", ratio); }
  float GetOverlapEstimation() const { return static_cast<float>(this->GetParam("OverlapEstimation")); }
  double GetLatency() const { return this->GetParam("Latency"); }
  // Slam::GetDebugArray (Slam.cxx:635-657); needs SetKeepMatchDebug(true)
  std::unordered_map<std::string, std::vector<double>> GetDebugArray() const
  {
    std::unordered_map<std::string, std::vector<double>> map;
    for (int loc = 0; loc < 2; ++loc)
      for (Keypoint k : KeypointTypes)
      {
        if (!loc && k == BLOB) continue;
        // size first (null buffers), then exactly that much
        const int have = lsa_slam_get_match_status(this->Handle, loc, k, nullptr, nullptr, 1 << 30);
        std::vector<std::uint8_t> st(have > 0 ? have : 0);
        std::vector<double> w(st.size());
        const int n = st.empty() ? 0 : lsa_slam_get_match_status(this->Handle, loc, k, st.data(), w.data(), static_cast<int>(st.size()));
        const std::string prefix = std::string(loc ? "Localization: " : "EgoMotion: ") + KeypointTypeNames.at(k);
        map[prefix + " matches"] = std::vector<double>(st.begin(), st.begin() + (n > 0 ? n : 0));
        w.resize(n > 0 ? n : 0);
        map[prefix + " weights"] = w;
      }
    return map;
  }
  const std::string& GetLastError() const { return this->LastError; }

  // ---- Slam::RunPoseGraphOptimization (Slam.cxx:355-477) on the device solver (lsa_slam_run_pose_graph_optimization): the
  // odometry chain of the log weighted by the inverse logged covariances, every pose free, plus a position prior per GPS fix
  // matched to a logged pose by time, behind inverse(gpsToSensorOffset).  As the reference: gpsToSensorOffset comes back as
  // the optimized first pose in the GPS frame, the trajectory comes back re-anchored on that pose and goes through
  // SetTrajectoryAndRebuildMaps.  Needs SetLoggingTimeout(!= 0) while the frames were added.  When it cannot -- no keypoint
  // log, fewer than two poses or fixes, times that do not overlap, no fix within 0.1 s of a pose, a covariance that is not
  // positive definite -- it says why once on stderr and in GetLastError(), and changes nothing.  A g2o file is not written.
  // The third form takes the solver's parameters (params.apply decides whether the maps are rebuilt), a time offset added to
  // the logged times before they are compared with the fixes', and gives the solver's summary and the optimized poses.
#ifdef LSA_HAVE_EIGEN
  void RunPoseGraphOptimization(const std::vector<Transform>& gpsPositions, const std::vector<std::array<double, 9>>& gpsCovariances, Eigen::Isometry3d& gpsToSensorOffset,
                                const std::string& g2oFileName = "")
  {
    std::array<double, 16> offset = Transform(gpsToSensorOffset).matrix;
    this->RunPoseGraphOptimization(gpsPositions, gpsCovariances, offset, g2oFileName);
    gpsToSensorOffset = Transform(offset).GetIsometry();
  }
#endif
  void RunPoseGraphOptimization(const std::vector<Transform>& gpsPositions, const std::vector<std::array<double, 9>>& gpsCovariances, std::array<double, 16>& gpsToSensorOffset,
                                const std::string& g2oFileName = "")
  {
    if (!g2oFileName.empty()) this->WarnOnce("RunPoseGraphOptimization (g2o file)", "no g2o file is written: the graph is solved on the device");
    lsa_pgo_params_t params;
    lsa_pgo_params_init(&params);
    params.odometry_information = 1;  // the reference's rule: the inverse of the logged covariance
    params.apply = 1;
    this->RunPoseGraphOptimization(gpsPositions, gpsCovariances, gpsToSensorOffset, params, 0., nullptr);
  }
  std::vector<Transform> RunPoseGraphOptimization(const std::vector<Transform>& gpsPositions, const std::vector<std::array<double, 9>>& gpsCovariances,
                                                  std::array<double, 16>& gpsToSensorOffset, const lsa_pgo_params_t& params, double timeOffset = 0.,
                                                  lsa_pgo_result_t* summary = nullptr)
  {
    return this->RunPoseGraphOptimization(gpsPositions, gpsCovariances, gpsToSensorOffset, params, DefaultRobustParameters(), timeOffset, summary, nullptr);
  }
  // ... under a robust loss on the GPS priors (robust.prior_loss / prior_scale; lsa_slam_run_pose_graph_optimization_robust): a fix
  // tens of metres off is discounted instead of bending the track.  fixVerdicts: per fix {chi2, weight} at the optimized poses,
  // weight -1 for a fix that matched no pose.  Geman-McClure and Tukey find the minimum nearest the logged odometry.
  using RobustParameters = lsa_pgo_robust_t;
  struct ConstraintVerdict
  {
    double chi2, weight;
  };
  static RobustParameters DefaultRobustParameters()
  {
    RobustParameters r;
    lsa_pgo_robust_init(&r);
    return r;
  }
  std::vector<Transform> RunPoseGraphOptimization(const std::vector<Transform>& gpsPositions, const std::vector<std::array<double, 9>>& gpsCovariances,
                                                  std::array<double, 16>& gpsToSensorOffset, const lsa_pgo_params_t& params, const RobustParameters& robust,
                                                  double timeOffset = 0., lsa_pgo_result_t* summary = nullptr, std::vector<ConstraintVerdict>* fixVerdicts = nullptr)
  {
    std::vector<Transform> poses = this->GetTrajectory();
    std::vector<double> rows((poses.size() + 1) * 17), times(gpsPositions.size()), xyz(gpsPositions.size() * 3), cov(gpsPositions.size() * 9);
    lsa_pgo_result_t result;
    std::memset(&result, 0, sizeof(result));
    int rc = LSA_E_ARG;
    if (gpsCovariances.size() != gpsPositions.size()) this->LastError = "RunPoseGraphOptimization: as many covariances as GPS positions";
    else
    {
      for (std::size_t f = 0; f < gpsPositions.size(); ++f)
      {
        times[f] = gpsPositions[f].time;
        xyz[3 * f] = gpsPositions[f].x(); xyz[3 * f + 1] = gpsPositions[f].y(); xyz[3 * f + 2] = gpsPositions[f].z();
        std::memcpy(cov.data() + 9 * f, gpsCovariances[f].data(), 9 * sizeof(double));
      }
      std::array<double, 16> offset = gpsToSensorOffset;
      std::vector<double> verdict(2 * gpsPositions.size());
      rc = lsa_slam_run_pose_graph_optimization_robust(this->Handle, times.data(), xyz.data(), cov.data(), static_cast<int>(gpsPositions.size()), offset.data(), timeOffset,
                                                       &params, &robust, rows.data(), static_cast<int>(poses.size()), &result, verdict.data());
      if (fixVerdicts)
      {
        fixVerdicts->clear();
        for (std::size_t f = 0; rc >= 0 && f < gpsPositions.size(); ++f) fixVerdicts->push_back(ConstraintVerdict{verdict[2 * f], verdict[2 * f + 1]});
      }
      this->LastError = rc < 0 ? std::string("RunPoseGraphOptimization: ") + lsa_slam_last_error(this->Handle) : std::string();
      if (rc >= 0) gpsToSensorOffset = offset;
    }
    if (rc < 0)
    {
      result.termination = rc;
      const std::size_t colon = this->LastError.find(": ");
      std::fprintf(stderr, "\033[1;33m[WARNING] LidarSlam::Slam::RunPoseGraphOptimization: %s; maps and trajectory are left unchanged\033[0m\n",
                   this->LastError.substr(colon == std::string::npos ? 0 : colon + 2).c_str());
    }
    if (summary) *summary = result;
    if (rc < 0) return {};
    for (std::size_t i = 0; i < poses.size(); ++i) std::memcpy(poses[i].matrix.data(), rows.data() + 17 * i, 16 * sizeof(double));
    return poses;
  }
  // ---- a corrected trajectory brought back (Slam.cxx:404-477, everything after the optimizer): the logged poses are
  // replaced by `poses` (as many as GetTrajectory() gives, each with its logged time), every logged frame's keypoints are
  // re-projected under them, the maps are rebuilt from the aggregate and rolled onto the last frame, Tworld / PreviousTworld
  // are set.  Needs SetLoggingTimeout(!= 0) while the frames were added.  A failure goes through GetLastError() and
  // changes nothing.
  void SetTrajectoryAndRebuildMaps(const std::vector<Transform>& poses)
  {
    std::vector<double> rows(poses.size() * 17);
    for (std::size_t i = 0; i < poses.size(); ++i)
    {
      std::memcpy(rows.data() + 17 * i, poses[i].matrix.data(), 16 * sizeof(double));
      rows[17 * i + 16] = poses[i].time;
    }
    const int rc = lsa_slam_set_trajectory_and_rebuild_maps(this->Handle, rows.data(), static_cast<int>(poses.size()));
    this->LastError = rc < 0 ? std::string("SetTrajectoryAndRebuildMaps: ") + lsa_slam_last_error(this->Handle) : std::string();
  }
  // ---- loop closure: the constraint an optimizer takes.  Logged frame `query` is registered against the logged keypoints
  // around logged frame `revisited` (indices into GetTrajectory()): a sub-map from the frames revisited -+
  // params.revisited_half_window under the logged poses, the ICP-LM loop of the localization from `guess` (the world pose of
  // query's BASE; nullptr = its logged pose) on the device, nothing but the result coming back.  The frame path does not
  // notice the call.  result.relative = inv(pose[revisited]) * result.world is the pose-graph edge revisited -> query,
  // result.covariance its uncertainty; result.status is 0 (registered) or 1 (too few matches: world = the guess).  When it
  // cannot -- no keypoint log, windows that overlap, an index outside the log -- nothing is changed, GetLastError() says
  // why and result.status is the negative LSA_E_* code.
  using LoopClosureParameters = lsa_loop_closure_params_t;
  using LoopClosureRegistration = lsa_loop_closure_result_t;
  static LoopClosureParameters DefaultLoopClosureParameters()
  {
    LoopClosureParameters p;
    lsa_loop_closure_params_init(&p);
    return p;
  }
  LoopClosureRegistration RegisterLoggedFrames(std::size_t query, std::size_t revisited, const LoopClosureParameters& params = DefaultLoopClosureParameters(),
                                               const Transform* guess = nullptr)
  {
    LoopClosureRegistration result;
    std::memset(&result, 0, sizeof(result));
    const int rc = lsa_slam_register_logged_frames(this->Handle, static_cast<int>(query), static_cast<int>(revisited), &params, guess ? guess->matrix.data() : nullptr, &result);
    this->LastError = rc < 0 ? std::string("RegisterLoggedFrames: ") + lsa_slam_last_error(this->Handle) : std::string();
    if (rc < 0) result.status = rc;
    return result;
  }
  // ---- place recognition: the logged frames before `query` that LOOK like it, whatever the drifted trajectory says about
  // where they are -- polar height descriptors of the logged keypoints, built and compared on the device, exhaustively
  // (lsa_slam_recognize_place).  Best first; candidate.yaw is the turn about z between the two frames, so a start guess for
  // RegisterLoggedFrames(query, candidate.frame, ...) is pose[candidate.frame] * Rz(candidate.yaw).  Empty when there is
  // none or when it cannot (GetLastError() says why).
  using PlaceSearchParameters = lsa_place_search_t;
  using PlaceCandidate = lsa_place_candidate_t;
  static PlaceSearchParameters DefaultPlaceSearchParameters()
  {
    PlaceSearchParameters p;
    lsa_place_search_init(&p);
    return p;
  }
  std::vector<PlaceCandidate> RecognizePlace(std::size_t query, const PlaceSearchParameters& params = DefaultPlaceSearchParameters(), std::size_t maxCandidates = 5)
  {
    std::vector<PlaceCandidate> found(maxCandidates);
    const int rc = lsa_slam_recognize_place(this->Handle, static_cast<int>(query), &params, found.data(), static_cast<int>(maxCandidates));
    this->LastError = rc < 0 ? std::string("RecognizePlace: ") + lsa_slam_last_error(this->Handle) : std::string();
    found.resize(static_cast<std::size_t>(rc > 0 ? rc : 0));
    return found;
  }
  // ---- place recognition against the MAPS: where in the maps (LoadMapsFromPCD, or the maps this object built) does the
  // last frame belong, when nobody can say -- a robot switched on somewhere inside its map, a localization that lost its
  // matches.  The maps are described as seen from each of `viewpoints` (positions in the maps' frame; the BASE is assumed
  // level there) and the last frame's descriptor is searched among them, on the device (lsa_slam_recognize_place_in_maps).
  // Best first; candidate.guess = Translation(viewpoint) * Rz(yaw) is what SetWorldTransformFromGuess takes -- the call
  // itself does not move the pose.  Needs one AddFrame since construction, Reset or SetWorldTransformFromGuess.  Empty when
  // there is none or when it cannot (GetLastError() says why).  Without viewpoints: the positions of GetTrajectory().
  using MapPlaceSearchParameters = lsa_map_place_search_t;
  using MapPlaceCandidate = lsa_map_place_candidate_t;
  using MapPlaceSummary = lsa_map_place_summary_t;
  static MapPlaceSearchParameters DefaultMapPlaceSearchParameters()
  {
    MapPlaceSearchParameters p;
    lsa_map_place_search_init(&p);
    return p;
  }
  std::vector<MapPlaceCandidate> RecognizePlaceInMaps(const std::vector<std::array<double, 3>>& viewpoints,
                                                      const MapPlaceSearchParameters& params = DefaultMapPlaceSearchParameters(), std::size_t maxCandidates = 5,
                                                      MapPlaceSummary* summary = nullptr)
  {
    std::vector<MapPlaceCandidate> found(maxCandidates);
    const int rc = lsa_slam_recognize_place_in_maps(this->Handle, viewpoints.empty() ? nullptr : viewpoints.front().data(), static_cast<int>(viewpoints.size()), &params,
                                                    found.data(), static_cast<int>(maxCandidates), summary);
    this->LastError = rc < 0 ? std::string("RecognizePlaceInMaps: ") + lsa_slam_last_error(this->Handle) : std::string();
    found.resize(static_cast<std::size_t>(rc > 0 ? rc : 0));
    return found;
  }
  std::vector<MapPlaceCandidate> RecognizePlaceInMaps(const MapPlaceSearchParameters& params = DefaultMapPlaceSearchParameters(), std::size_t maxCandidates = 5,
                                                      MapPlaceSummary* summary = nullptr)
  {
    std::vector<std::array<double, 3>> viewpoints;
    for (const Transform& t : this->GetTrajectory()) viewpoints.push_back({t.matrix[3], t.matrix[7], t.matrix[11]});
    if (viewpoints.empty())
    {
      this->LastError = "RecognizePlaceInMaps: the trajectory is empty and no viewpoints were given";
      return {};
    }
    return this->RecognizePlaceInMaps(viewpoints, params, maxCandidates, summary);
  }
  // ---- pose-graph optimization of the logged trajectory on the device (lsa_slam_optimize_logged_trajectory): the odometry
  // chain of the log, pose 0 fixed, plus the loop edges given -- LoopClosureEdge(revisited, query, registration) makes one from
  // what RegisterLoggedFrames returned.  Returns the optimized poses with their logged times (empty when it cannot:
  // GetLastError() says why and summary->termination is the negative LSA_E_* code); with params.apply != 0 they have gone through
  // SetTrajectoryAndRebuildMaps as well, with 0 nothing the frame path reads is touched.  RunPoseGraphOptimization above, the
  // reference's entry point with GPS positions, runs on the same solver with every pose free and the positions as priors.
  using PoseGraphEdge = lsa_pgo_edge_t;
  using PoseGraphParameters = lsa_pgo_params_t;
  using PoseGraphSummary = lsa_pgo_result_t;
  static PoseGraphParameters DefaultPoseGraphParameters()
  {
    PoseGraphParameters p;
    lsa_pgo_params_init(&p);
    return p;
  }
  // information = inverse(registration.covariance); false when that is not positive definite (the edge is left zeroed)
  static bool LoopClosureEdge(std::size_t revisited, std::size_t query, const LoopClosureRegistration& registration, PoseGraphEdge& edge)
  {
    std::memset(&edge, 0, sizeof(edge));
    edge.from = static_cast<int>(revisited);
    edge.to = static_cast<int>(query);
    std::memcpy(edge.relative, registration.relative, sizeof(edge.relative));
    return lsa_pgo_information_from_covariance(registration.covariance, edge.information) == 0;
  }
  std::vector<Transform> OptimizeLoggedTrajectory(const std::vector<PoseGraphEdge>& loopEdges, const PoseGraphParameters& params = DefaultPoseGraphParameters(),
                                                  PoseGraphSummary* summary = nullptr)
  {
    return this->OptimizeLoggedTrajectory(loopEdges, params, DefaultRobustParameters(), summary, nullptr);
  }
  // ... under a robust loss on the loop edges (robust.edge_loss / edge_scale; lsa_slam_optimize_logged_trajectory_robust): a false
  // loop edge is discounted instead of bending the trajectory; the odometry chain is never discounted.  loopVerdicts: per loop
  // edge {chi2, weight} at the optimized poses -- under Tukey a weight of 0 says the edge was disregarded.
  std::vector<Transform> OptimizeLoggedTrajectory(const std::vector<PoseGraphEdge>& loopEdges, const PoseGraphParameters& params, const RobustParameters& robust,
                                                  PoseGraphSummary* summary = nullptr, std::vector<ConstraintVerdict>* loopVerdicts = nullptr)
  {
    std::vector<Transform> poses = this->GetTrajectory();
    std::vector<double> rows((poses.size() + 1) * 17), verdict(2 * loopEdges.size() + 2);
    PoseGraphSummary result;
    std::memset(&result, 0, sizeof(result));
    const int rc = lsa_slam_optimize_logged_trajectory_robust(this->Handle, loopEdges.empty() ? nullptr : loopEdges.data(), static_cast<int>(loopEdges.size()), &params, &robust,
                                                              rows.data(), static_cast<int>(poses.size()), &result, verdict.data());
    if (loopVerdicts)
    {
      loopVerdicts->clear();
      for (std::size_t k = 0; rc >= 0 && k < loopEdges.size(); ++k) loopVerdicts->push_back(ConstraintVerdict{verdict[2 * k], verdict[2 * k + 1]});
    }
    this->LastError = rc < 0 ? std::string("OptimizeLoggedTrajectory: ") + lsa_slam_last_error(this->Handle) : std::string();
    if (rc < 0) result.termination = rc;
    if (summary) *summary = result;
    if (rc < 0) return {};
    for (std::size_t i = 0; i < poses.size(); ++i) std::memcpy(poses[i].matrix.data(), rows.data() + 17 * i, 16 * sizeof(double));
    return poses;
  }
  // ---- every loop closure of the log.  DetectLoopClosures: where did this drive revisit itself -- RecognizePlace for every
  // query of a set (first_query, first_query + query_stride, ... <= last_query; < 0: the last logged frame) with per_query
  // (1..16) candidates each, in one pass on the device (lsa_slam_detect_loop_closures).  The queries ascending, each query's
  // candidates best first; empty when there is none or when it cannot (GetLastError() says why).
  using LoopDetectionParameters = lsa_loop_detect_t;
  using LoopCandidate = lsa_loop_candidate_t;
  using LoopReport = lsa_loop_report_t;
  static LoopDetectionParameters DefaultLoopDetectionParameters()
  {
    LoopDetectionParameters p;
    lsa_loop_detect_init(&p);
    return p;
  }
  std::vector<LoopCandidate> DetectLoopClosures(const LoopDetectionParameters& detect = DefaultLoopDetectionParameters())
  {
    const int n = lsa_slam_logged_frames(this->Handle);
    const int last = detect.last_query < 0 ? n - 1 : detect.last_query;
    const long long room = detect.query_stride >= 1 && detect.per_query >= 1 && last >= detect.first_query
                             ? ((static_cast<long long>(last) - detect.first_query) / detect.query_stride + 1) * detect.per_query : 0;
    std::vector<LoopCandidate> found(static_cast<std::size_t>(room > 0 ? room : 1));
    const int rc = lsa_slam_detect_loop_closures(this->Handle, &detect, found.data(), static_cast<int>(room));
    this->LastError = rc < 0 ? std::string("DetectLoopClosures: ") + lsa_slam_last_error(this->Handle) : std::string();
    found.resize(static_cast<std::size_t>(rc > 0 ? rc : 0));
    return found;
  }
  // CloseLoops: fix it -- DetectLoopClosures, RegisterLoggedFrames(query, frame, loopParams, pose[frame] * Rz(yaw)) for every
  // candidate under the logged poses, a LoopClosureEdge for every registration with status 0 and a positive definite
  // covariance, one OptimizeLoggedTrajectory over them under `robust` (a false place match is discounted, not obeyed), applied
  // where pgoParams.apply != 0 (lsa_slam_close_loops).  Returns the optimized poses; `reports` gets one entry per candidate:
  // its registration, its edge's index (-1: none came of it) and its verdict {chi2, weight}.  Without a candidate or an edge
  // nothing is solved or changed: the logged poses come back, summary->message says so, GetLastError() is empty.  Empty when it
  // cannot (GetLastError() says why and summary->termination is the negative LSA_E_* code).
  std::vector<Transform> CloseLoops(const LoopDetectionParameters& detect, const LoopClosureParameters& loopParams, const PoseGraphParameters& pgoParams,
                                    const RobustParameters& robust, PoseGraphSummary* summary = nullptr, std::vector<LoopReport>* reports = nullptr)
  {
    std::vector<Transform> poses = this->GetTrajectory();
    const int last = detect.last_query < 0 ? static_cast<int>(poses.size()) - 1 : detect.last_query;
    const long long room = detect.query_stride >= 1 && detect.per_query >= 1 && last >= detect.first_query
                             ? ((static_cast<long long>(last) - detect.first_query) / detect.query_stride + 1) * detect.per_query : 0;
    std::vector<LoopReport> rep(static_cast<std::size_t>(room > 0 ? room : 1));
    std::vector<double> rows((poses.size() + 1) * 17);
    PoseGraphSummary result;
    std::memset(&result, 0, sizeof(result));
    const int rc = lsa_slam_close_loops(this->Handle, &detect, &loopParams, &pgoParams, &robust, rows.data(), static_cast<int>(poses.size()), &result, rep.data(),
                                        static_cast<int>(room));
    this->LastError = rc < 0 ? std::string("CloseLoops: ") + lsa_slam_last_error(this->Handle) : std::string();
    if (rc < 0) result.termination = rc;
    if (summary) *summary = result;
    rep.resize(static_cast<std::size_t>(rc > 0 ? rc : 0));
    if (reports) *reports = rep;
    if (rc < 0) return {};
    for (std::size_t i = 0; i < poses.size(); ++i) std::memcpy(poses[i].matrix.data(), rows.data() + 17 * i, 16 * sizeof(double));
    return poses;
  }
  // The logged frame to try a loop closure of `query` against BY POSITION: among the frames at least minTravelled metres
  // back along GetTrajectory() and within maxDistance metres of query's position, the nearest; -1 when there is none.  Host
  // only.  By appearance: RecognizePlace above.
  int FindLoopClosureCandidate(std::size_t query, double minTravelled, double maxDistance) const
  {
    const int n = lsa_slam_get_trajectory(this->Handle, nullptr, nullptr, 0);
    std::vector<double> rows(static_cast<std::size_t>(n > 0 ? n : 0) * 17);
    if (n > 0) lsa_slam_get_trajectory(this->Handle, rows.data(), nullptr, n);
    const int found = lsa_loop_closure_candidate(rows.data(), n, static_cast<int>(query), minTravelled, maxDistance);
    return found < 0 ? -1 : found;
  }
  // the raw keypoints (BASE, not undistorted) logged with pose `frame` of GetTrajectory()
  PointCloud::Ptr GetLoggedKeypoints(Keypoint k, std::size_t frame)
  {
    return this->Fetch([&](lsa_point_t* out, int cap) { return std::min(cap, lsa_slam_get_logged_keypoints(this->Handle, static_cast<int>(frame), k, out, cap)); },
                       this->BaseFrameId);
  }
  // ---- the keypoint maps as PCD files (Slam.cxx:504-543): <prefix>edges.pcd, <prefix>planes.pcd, <prefix>blobs.pcd.  A
  // failure is reported through GetLastError(); the first call of each per object says on stderr what it wrote or loaded.
  void SaveMapsToPCD(const std::string& filePrefix, PCDFormat pcdFormat = PCDFormat::BINARY_COMPRESSED, bool filtered = true) const
  {
    const int rc = lsa_slam_save_maps_pcd(this->Handle, filePrefix.c_str(), static_cast<int>(pcdFormat), filtered ? 1 : 0);
    this->ReportMapIO("SaveMapsToPCD", "saved to", filePrefix, rc);
  }
  void LoadMapsFromPCD(const std::string& filePrefix, bool resetMaps = true)
  {
    const int rc = lsa_slam_load_maps_pcd(this->Handle, filePrefix.c_str(), resetMaps ? 1 : 0, -1.);
    this->ReportMapIO("LoadMapsFromPCD", "loaded from", filePrefix, rc);
  }
  // the library's parameter "LoggingStorage".  All five values are accepted and mean the same thing here: the keypoint
  // log is kept uncompressed in the device's memory (32 B a keypoint); nothing is compressed
  LSA_SLAM_ENUM_PARAM(LoggingStorage, PointCloudStorageType)
  // ---- wheel odometer / IMU gravity constraints (Slam.h:331-343, Slam.cxx:223-227, 1582-1598): the terms enter every ICP
  // iteration of the localization solve and its covariance; the weights and the time offset are the library's
  // parameters WheelOdomWeight, GravityWeight, SensorTimeOffset
  LSA_SLAM_PARAM(WheelOdomWeight, double)
  LSA_SLAM_PARAM(GravityWeight, double)
  LSA_SLAM_PARAM(SensorTimeOffset, double)  // both sensors' offset: the LiDAR time minus it is the sensors' time
  void AddGravityMeasurement(const SensorConstraints::GravityMeasurement& m)
  {
    const double acc[3] = {m.Acceleration[0], m.Acceleration[1], m.Acceleration[2]};
    lsa_slam_add_gravity_measurement(this->Handle, m.Time, acc);
    if (this->GetGravityWeight() <= 1e-6) this->WarnOnce("AddGravityMeasurement", "stored; no constraint while the weight is 0");
  }
  void AddWheelOdomMeasurement(const SensorConstraints::WheelOdomMeasurement& m)
  {
    lsa_slam_add_wheel_odom_measurement(this->Handle, m.Time, m.Distance);
    if (this->GetWheelOdomWeight() <= 1e-6) this->WarnOnce("AddWheelOdomMeasurement", "stored; no constraint while the weight is 0");
  }
  // measurements and the current terms cleared, time offset 0; the gravity reference and the odometer's baseline stay
  void ClearSensorMeasurements() { lsa_slam_clear_sensor_measurements(this->Handle); }

  // ---- general parameters (Slam.h:201-232)
  void SetNbThreads(int) {}  // OpenMP thread count of the reference: meaningless on the device path
  int GetNbThreads() const { return 1; }
  void SetVerbosity(int v) { this->Verbosity = v; }
  int GetVerbosity() const { return this->Verbosity; }
  LSA_SLAM_PARAM(UseBlobs, bool)
  LSA_SLAM_ENUM_PARAM(EgoMotion, EgoMotionMode)
  LSA_SLAM_ENUM_PARAM(Undistortion, UndistortionMode)
  LSA_SLAM_ENUM_PARAM(MapUpdate, MappingMode)
  LSA_SLAM_PARAM(KeepMatchDebug, bool)
  LSA_SLAM_PARAM(LoggingTimeout, double)
  // Slam.h:239-245: the extraction runs inside the library, so what is taken from the extractor object is its
  // parameters (and its azimuthal resolution when it has one); the object is kept for GetKeyPointsExtractor
  using KeypointExtractorPtr = std::shared_ptr<SpinningSensorKeypointExtractor>;
  void SetKeyPointsExtractor(KeypointExtractorPtr extractor, std::uint8_t deviceId = 0)
  {
    if (!extractor) return;
    const std::pair<const char*, double> values[] = {
      {"NeighborWidth", extractor->GetNeighborWidth()}, {"MinDistanceToSensor", extractor->GetMinDistanceToSensor()},
      {"MinBeamSurfaceAngle", extractor->GetMinBeamSurfaceAngle()}, {"PlaneSinAngleThreshold", extractor->GetPlaneSinAngleThreshold()},
      {"EdgeSinAngleThreshold", extractor->GetEdgeSinAngleThreshold()}, {"EdgeDepthGapThreshold", extractor->GetEdgeDepthGapThreshold()},
      {"EdgeSaliencyThreshold", extractor->GetEdgeSaliencyThreshold()}, {"EdgeIntensityGapThreshold", extractor->GetEdgeIntensityGapThreshold()}};
    for (const auto& v : values) lsa_slam_set_extractor_param(this->Handle, deviceId, v.first, v.second);
    if (extractor->GetAzimuthalResolution() > 0.f)
      lsa_slam_set_extractor_param(this->Handle, deviceId, "AzimuthalResolution", extractor->GetAzimuthalResolution());
    this->KeyPointsExtractors[deviceId] = extractor;
  }
  KeypointExtractorPtr GetKeyPointsExtractor(std::uint8_t deviceId = 0) const
  {
    const auto it = this->KeyPointsExtractors.find(deviceId);
    return it != this->KeyPointsExtractors.end() ? it->second : KeypointExtractorPtr();
  }
  std::map<std::uint8_t, KeypointExtractorPtr> GetKeyPointsExtractors() const { return this->KeyPointsExtractors; }
  void SetKeyPointsExtractors(const std::map<std::uint8_t, KeypointExtractorPtr>& extractors)
  {
    for (const auto& kv : extractors) this->SetKeyPointsExtractor(kv.second, kv.first);
  }
  // Slam.h:249-250 (row-major 4x4)
  void SetBaseToLidarOffset(const std::array<double, 16>& transform, std::uint8_t deviceId = 0)
  {
    lsa_slam_set_base_to_lidar_offset(this->Handle, transform.data(), deviceId);
  }
  std::array<double, 16> GetBaseToLidarOffset(std::uint8_t deviceId = 0) const
  {
    std::array<double, 16> t{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    lsa_slam_get_base_to_lidar_offset(this->Handle, t.data(), deviceId);
    return t;
  }
#ifdef LSA_HAVE_EIGEN
  void SetBaseToLidarOffset(const Eigen::Isometry3d& transform, std::uint8_t deviceId = 0)
  {
    std::array<double, 16> t{};
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) t[r * 4 + c] = transform.matrix()(r, c);
    this->SetBaseToLidarOffset(t, deviceId);
  }
#endif
  // confidence estimator on the motion (Slam.h:385-394): {linear, angular} limits
  void SetVelocityLimits(const std::array<float, 2>& l) { this->SetParam("VelocityLimitLinear", l[0]); this->SetParam("VelocityLimitAngular", l[1]); }
  std::array<float, 2> GetVelocityLimits() const { return {{static_cast<float>(this->GetParam("VelocityLimitLinear")), static_cast<float>(this->GetParam("VelocityLimitAngular"))}}; }
  void SetAccelerationLimits(const std::array<float, 2>& l) { this->SetParam("AccelerationLimitLinear", l[0]); this->SetParam("AccelerationLimitAngular", l[1]); }
  std::array<float, 2> GetAccelerationLimits() const { return {{static_cast<float>(this->GetParam("AccelerationLimitLinear")), static_cast<float>(this->GetParam("AccelerationLimitAngular"))}}; }
#ifdef LSA_HAVE_EIGEN
  // the reference's own argument type (Slam.h:385-392)
  void SetVelocityLimits(const Eigen::Array2f& l) { this->SetVelocityLimits(std::array<float, 2>{{l(0), l(1)}}); }
  void SetAccelerationLimits(const Eigen::Array2f& l) { this->SetAccelerationLimits(std::array<float, 2>{{l(0), l(1)}}); }
#endif
  LSA_SLAM_PARAM(TimeWindowDuration, float)
  bool GetComplyMotionLimits() const { return this->GetParam("ComplyMotionLimits") != 0.; }
  void SetBaseFrameId(const std::string& s) { this->BaseFrameId = s; }
  std::string GetBaseFrameId() const { return this->BaseFrameId; }
  void SetWorldFrameId(const std::string& s) { this->WorldFrameId = s; }
  std::string GetWorldFrameId() const { return this->WorldFrameId; }

  // ---- optimisation parameters (Slam.h:262-340)
  LSA_SLAM_PARAM(TwoDMode, bool)
  LSA_SLAM_PARAM(EgoMotionLMMaxIter, unsigned int)
  LSA_SLAM_PARAM(EgoMotionICPMaxIter, unsigned int)
  LSA_SLAM_PARAM(EgoMotionMaxNeighborsDistance, double)
  LSA_SLAM_PARAM(EgoMotionEdgeNbNeighbors, unsigned int)
  LSA_SLAM_PARAM(EgoMotionEdgeMinNbNeighbors, unsigned int)
  LSA_SLAM_PARAM(EgoMotionPlaneNbNeighbors, unsigned int)
  LSA_SLAM_PARAM(EgoMotionPlanarityThreshold, double)
  LSA_SLAM_PARAM(EgoMotionEdgeMaxModelError, double)
  LSA_SLAM_PARAM(EgoMotionPlaneMaxModelError, double)
  LSA_SLAM_PARAM(EgoMotionInitSaturationDistance, double)
  LSA_SLAM_PARAM(EgoMotionFinalSaturationDistance, double)
  LSA_SLAM_PARAM(LocalizationLMMaxIter, unsigned int)
  LSA_SLAM_PARAM(LocalizationICPMaxIter, unsigned int)
  LSA_SLAM_PARAM(LocalizationMaxNeighborsDistance, double)
  LSA_SLAM_PARAM(LocalizationEdgeNbNeighbors, unsigned int)
  LSA_SLAM_PARAM(LocalizationEdgeMinNbNeighbors, unsigned int)
  LSA_SLAM_PARAM(LocalizationPlaneNbNeighbors, unsigned int)
  LSA_SLAM_PARAM(LocalizationPlanarityThreshold, double)
  LSA_SLAM_PARAM(LocalizationEdgeMaxModelError, double)
  LSA_SLAM_PARAM(LocalizationPlaneMaxModelError, double)
  LSA_SLAM_PARAM(LocalizationBlobNbNeighbors, unsigned int)
  LSA_SLAM_PARAM(LocalizationInitSaturationDistance, double)
  LSA_SLAM_PARAM(LocalizationFinalSaturationDistance, double)

  // ---- keyframes and maps (Slam.h:360-378)
  LSA_SLAM_PARAM(KfDistanceThreshold, double)
  LSA_SLAM_PARAM(KfAngleThreshold, double)
  void SetVoxelGridLeafSize(Keypoint k, double size)
  {
    this->SetParam(k == EDGE ? "VoxelGridLeafSizeEdges" : k == PLANE ? "VoxelGridLeafSizePlanes" : "VoxelGridLeafSizeBlobs", size);
  }
  void SetVoxelGridSize(int size) { this->SetParam("VoxelGridSize", size); }
  void SetVoxelGridResolution(double r) { this->SetParam("VoxelGridResolution", r); }
  void SetVoxelGridMinFramesPerVoxel(unsigned int n) { this->SetParam("VoxelGridMinFramesPerVoxel", n); }
  void SetVoxelGridDecayingThreshold(double d) { this->SetParam("VoxelGridDecayingThreshold", d); }
  void SetVoxelGridSamplingMode(Keypoint, SamplingMode sm) { this->SetParam("VoxelGridSamplingMode", static_cast<int>(sm)); }
  SamplingMode GetVoxelGridSamplingMode(Keypoint) { return static_cast<SamplingMode>(static_cast<int>(this->GetParam("VoxelGridSamplingMode"))); }
  double GetVoxelGridDecayingThreshold() { return this->GetParam("VoxelGridDecayingThreshold"); }
  // Slam::ClearMaps (Slam.cxx): empties the three keypoint maps, poses and parameters stay
  void ClearMaps() { lsa_slam_clear_maps(this->Handle); }

  // ---- the dense point-cloud map (not in the reference, whose wrappers voxelize GetRegisteredFrame themselves): the
  // registered frame of every AddFrame (mode 1) or of every keyframe (mode 2) goes into a voxel hash table on the device,
  // one point per voxel of SetDenseMapLeafSize metres (default 0.1).  minFrames: only voxels seen in that many frames, the
  // MinFramesPerVoxel idea (a passing car touches a voxel in a frame or two, a wall in many).  Cleared by Reset, ClearMaps
  // and every applied trajectory.  A failure is reported through GetLastError().
  void SetDenseMap(int mode) { this->SetParam("DenseMap", mode); }
  int GetDenseMapMode() const { return static_cast<int>(this->GetParam("DenseMap")); }
  void SetDenseMapLeafSize(double size) { this->SetParam("DenseMapLeafSize", size); }
  double GetDenseMapLeafSize() const { return this->GetParam("DenseMapLeafSize"); }
  // the size is asked for first, so the map is exported once and whole whatever its size; on a failure the cloud is empty
  PointCloud::Ptr GetDenseMap(int minFrames = 1)
  {
    PointCloud::Ptr pc(new PointCloud);
    pc->header.stamp = this->CurrentStamp;
    pc->header.frame_id = this->WorldFrameId;
    int n = lsa_slam_dense_map_size(this->Handle);
    if (n > 0)
    {
      pc->points.resize(static_cast<std::size_t>(n));
      n = lsa_slam_get_dense_map(this->Handle, minFrames, reinterpret_cast<lsa_point_t*>(pc->points.data()), nullptr, n);
      pc->points.resize(static_cast<std::size_t>(std::max(n, 0)));
    }
    this->LastError = n < 0 ? std::string("GetDenseMap: ") + lsa_slam_last_error(this->Handle) : std::string();
    return pc;
  }
  // What an applied trajectory (SetTrajectoryAndRebuildMaps, the pose-graph calls and CloseLoops with apply) does to the dense
  // map.  0, the default: it is cleared.  1: it is re-projected on the device -- one point per voxel, moved by new * inverse(old)
  // of the logged pose of the frame that measured it; not a rebuild from raw frames, so two neighbouring surface voxels may
  // merge and the voxel between them stay empty until it is seen again.  Reset, ClearMaps and ClearDenseMap clear either way.
  void SetDenseMapOnTrajectory(int mode) { this->SetParam("DenseMapOnTrajectory", mode); }
  int GetDenseMapOnTrajectory() const { return static_cast<int>(this->GetParam("DenseMapOnTrajectory")); }
  // per point of GetDenseMap(minFrames), in its order: the ordinal (count of inserted calls) of the frame that measured it
  std::vector<int> GetDenseMapSources(int minFrames = 1)
  {
    std::vector<int> out;
    int n = lsa_slam_dense_map_size(this->Handle);
    if (n > 0)
    {
      out.resize(static_cast<std::size_t>(n));
      n = lsa_slam_get_dense_map_sources(this->Handle, minFrames, out.data(), n);
      out.resize(static_cast<std::size_t>(std::max(n, 0)));
    }
    this->LastError = n < 0 ? std::string("GetDenseMapSources: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  // returns the points written (0 and no file for an empty map), negative on failure
  int SaveDenseMapToPCD(const std::string& path, PCDFormat pcdFormat = PCDFormat::BINARY_COMPRESSED, int minFrames = 1) const
  {
    const int rc = lsa_slam_save_dense_map_pcd(this->Handle, path.c_str(), static_cast<int>(pcdFormat), minFrames);
    this->LastError = rc < 0 ? std::string("SaveDenseMapToPCD: ") + lsa_slam_last_error(this->Handle) : std::string();
    return rc;
  }
  void ClearDenseMap()
  {
    const int rc = lsa_slam_clear_dense_map(this->Handle);
    this->LastError = rc < 0 ? std::string("ClearDenseMap: ") + lsa_slam_last_error(this->Handle) : std::string();
  }
  // Free space: with SetDenseMapCarve(1) the ray of every inserted point, from where the sensor stood when it measured the
  // point to CarveMarginLeaves voxels before it (CarveRange metres at most, every CarveStride-th point), is walked through the
  // voxel grid on the device, and a voxel it passes through that the same frame did not hit counts one miss for the frame.
  // maxMissRatio: only voxels with misses <= maxMissRatio * frames (below 0: all) -- what moved away is seen through more often
  // than it was seen.  PruneDenseMap removes the others from the table for good and returns their number (negative on failure).
  void SetDenseMapCarve(int on) { this->SetParam("DenseMapCarve", on); }
  int GetDenseMapCarve() const { return static_cast<int>(this->GetParam("DenseMapCarve")); }
  void SetDenseMapCarveRange(double metres) { this->SetParam("DenseMapCarveRange", metres); }
  void SetDenseMapCarveMarginLeaves(double leaves) { this->SetParam("DenseMapCarveMarginLeaves", leaves); }
  void SetDenseMapCarveStride(int stride) { this->SetParam("DenseMapCarveStride", stride); }
  PointCloud::Ptr GetDenseMap(int minFrames, double maxMissRatio)
  {
    PointCloud::Ptr pc(new PointCloud);
    pc->header.stamp = this->CurrentStamp;
    pc->header.frame_id = this->WorldFrameId;
    int n = lsa_slam_dense_map_size(this->Handle);
    if (n > 0)
    {
      pc->points.resize(static_cast<std::size_t>(n));
      n = lsa_slam_get_dense_map_filtered(this->Handle, minFrames, maxMissRatio, reinterpret_cast<lsa_point_t*>(pc->points.data()), nullptr, n);
      pc->points.resize(static_cast<std::size_t>(std::max(n, 0)));
    }
    this->LastError = n < 0 ? std::string("GetDenseMap: ") + lsa_slam_last_error(this->Handle) : std::string();
    return pc;
  }
  // per point of GetDenseMap(minFrames, maxMissRatio), in its order: the frames whose rays passed through its voxel
  std::vector<std::uint32_t> GetDenseMapMisses(int minFrames = 1, double maxMissRatio = -1.)
  {
    std::vector<std::uint32_t> out;
    int n = lsa_slam_dense_map_size(this->Handle);
    if (n > 0)
    {
      out.resize(static_cast<std::size_t>(n));
      n = lsa_slam_get_dense_map_misses(this->Handle, minFrames, maxMissRatio, out.data(), n);
      out.resize(static_cast<std::size_t>(std::max(n, 0)));
    }
    this->LastError = n < 0 ? std::string("GetDenseMapMisses: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  int SaveDenseMapToPCD(const std::string& path, PCDFormat pcdFormat, int minFrames, double maxMissRatio) const
  {
    const int rc = lsa_slam_save_dense_map_pcd_filtered(this->Handle, path.c_str(), static_cast<int>(pcdFormat), minFrames, maxMissRatio);
    this->LastError = rc < 0 ? std::string("SaveDenseMapToPCD: ") + lsa_slam_last_error(this->Handle) : std::string();
    return rc;
  }
  long long PruneDenseMap(int minFrames = 1, double maxMissRatio = 1.)
  {
    long long removed = 0;
    const int rc = lsa_slam_prune_dense_map(this->Handle, minFrames, maxMissRatio, &removed);
    this->LastError = rc < 0 ? std::string("PruneDenseMap: ") + lsa_slam_last_error(this->Handle) : std::string();
    return rc < 0 ? rc : removed;
  }
  // Normals: per point of GetDenseMap(minFrames, maxMissRatio), in its order, the eigenvector of the smallest eigenvalue of the
  // covariance of the kept points of the voxels within radiusLeaves (1 or 2) that pass the same filter, PCL's surface variation
  // as curvature and the number of those voxels; NaN (PCL's "no normal") below minNeighbors.  With orient the normal is turned
  // towards where the sensor stood when it measured the point (GetDenseMapViewpoints).  Computed on the device from the table
  // as it stands; nothing is stored.
  struct DenseNormal
  {
    float normal_x, normal_y, normal_z, curvature;
    std::uint32_t neighbors;
  };
  std::vector<DenseNormal> GetDenseMapNormals(int minFrames = 1, double maxMissRatio = -1., int radiusLeaves = 2, int minNeighbors = 5, bool orient = true)
  {
    static_assert(sizeof(DenseNormal) == sizeof(lsa_dense_normal_t), "DenseNormal is lsa_dense_normal_t");
    std::vector<DenseNormal> out;
    int n = lsa_slam_dense_map_size(this->Handle);
    if (n > 0)
    {
      out.resize(static_cast<std::size_t>(n));
      n = lsa_slam_get_dense_map_normals(this->Handle, minFrames, maxMissRatio, radiusLeaves, minNeighbors, orient ? 1 : 0, reinterpret_cast<lsa_dense_normal_t*>(out.data()), n);
      out.resize(static_cast<std::size_t>(std::max(n, 0)));
    }
    this->LastError = n < 0 ? std::string("GetDenseMapNormals: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  // GetDenseMap(minFrames, maxMissRatio) with the fields normal_x normal_y normal_z curvature behind every point
  int SaveDenseMapWithNormalsToPCD(const std::string& path, PCDFormat pcdFormat = PCDFormat::BINARY, int minFrames = 1, double maxMissRatio = -1., int radiusLeaves = 2,
                                   int minNeighbors = 5, bool orient = true) const
  {
    const int rc = lsa_slam_save_dense_map_pcd_normals(this->Handle, path.c_str(), static_cast<int>(pcdFormat), minFrames, maxMissRatio, radiusLeaves, minNeighbors, orient ? 1 : 0);
    this->LastError = rc < 0 ? std::string("SaveDenseMapWithNormalsToPCD: ") + lsa_slam_last_error(this->Handle) : std::string();
    return rc;
  }
  // float xyz per inserted frame since the map was last cleared: where the (first) sensor stood
  std::vector<float> GetDenseMapViewpoints()
  {
    int first = 0;
    int n = lsa_slam_get_dense_map_viewpoints(this->Handle, nullptr, 0, &first);
    std::vector<float> out(3 * static_cast<std::size_t>(std::max(n, 0)));
    if (n > 0) n = lsa_slam_get_dense_map_viewpoints(this->Handle, out.data(), n, &first);
    out.resize(3 * static_cast<std::size_t>(std::max(n, 0)));
    this->LastError = n < 0 ? std::string("GetDenseMapViewpoints: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  // The floor plan: the dense map rasterised on the device into cells of cellLeaves voxels -- elevation (the lowest kept point
  // of the cell), ground (the lowest elevation within groundRadius cells), and the state of nav_msgs/OccupancyGrid: 100
  // occupied (minObstacleVoxels voxels at least between minHeight and maxHeight above the ground), 0 free (the floor was seen
  // and nothing stands on it; what is higher than maxHeight is driven under), -1 unknown.  Only the voxels of
  // GetDenseMap(minFrames, maxMissRatio) count.  With useWindow the grid is exactly the window (metres, world frame), and is the
  // crop of the whole grid; without, the bounding box of the map.  Cells are row-major, row 0 is the lowest y, x fastest.
  struct DenseGridParams
  {
    int cellLeaves = 2, groundRadius = 2, minObstacleVoxels = 1, minFrames = 1;
    double minHeight = 0.2, maxHeight = 2.0, maxMissRatio = -1.;
    bool useWindow = false;
    double xMin = 0., yMin = 0., xMax = 0., yMax = 0.;
    DenseGridParams() {}  // (user-provided: the defaults above are used as default arguments inside the enclosing class)
  };
  struct DenseCell
  {
    float elevation, ground, top;  // NaN: not there
    std::uint32_t floor_voxels, obstacle_voxels;
  };
  struct DenseGrid
  {
    int cx0 = 0, cy0 = 0, width = 0, height = 0;         // in cells
    double resolution = 0., origin_x = 0., origin_y = 0.;  // metres: the cell's side, the world position of the corner of cell (0, 0)
    std::vector<DenseCell> cells;
    std::vector<std::int8_t> states;
  };
  void SetDenseMapGridMaxCells(double cells) { this->SetParam("DenseMapGridMaxCells", cells); }
  double GetDenseMapGridMaxCells() const { return this->GetParam("DenseMapGridMaxCells"); }
  DenseGrid GetDenseMapGrid(const DenseGridParams& params = DenseGridParams())
  {
    static_assert(sizeof(DenseCell) == sizeof(lsa_dense_cell_t), "DenseCell is lsa_dense_cell_t");
    const lsa_dense_grid_params_t p = GridParams(params);
    lsa_dense_grid_info_t info;
    DenseGrid out;
    // the extent is asked for first (no cell is computed for it), so the grid is handed out once and whole
    long long n = lsa_slam_get_dense_map_grid(this->Handle, &p, &info, nullptr, nullptr, 0);
    if (n > 0)
    {
      out.cells.resize(static_cast<std::size_t>(n));
      out.states.resize(static_cast<std::size_t>(n));
      n = lsa_slam_get_dense_map_grid(this->Handle, &p, &info, reinterpret_cast<lsa_dense_cell_t*>(out.cells.data()), out.states.data(), n);
    }
    if (n >= 0)
    {
      out.cx0 = info.cx0; out.cy0 = info.cy0; out.width = info.width; out.height = info.height;
      out.resolution = info.resolution; out.origin_x = info.origin_x; out.origin_y = info.origin_y;
    }
    out.cells.resize(static_cast<std::size_t>(std::max(n, 0ll)));
    out.states.resize(static_cast<std::size_t>(std::max(n, 0ll)));
    this->LastError = n < 0 ? std::string("GetDenseMapGrid: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  // the local costmap: the window of 2 * halfExtent metres a side around the current GetWorldTransform translation
  DenseGrid GetDenseMapGridAround(double halfExtent, DenseGridParams params = DenseGridParams())
  {
    const Transform t = this->GetWorldTransform();
    params.useWindow = true;
    params.xMin = t.matrix[3] - halfExtent; params.xMax = t.matrix[3] + halfExtent;
    params.yMin = t.matrix[7] - halfExtent; params.yMax = t.matrix[7] + halfExtent;
    return this->GetDenseMapGrid(params);
  }
  // <prefix>.pgm and <prefix>.yaml for map_server: occupied 0, free 254, unknown 205; the number of cells, 0 and no files for none
  long long SaveDenseMapGrid(const std::string& prefix, const DenseGridParams& params = DenseGridParams()) const
  {
    const lsa_dense_grid_params_t p = GridParams(params);
    const long long rc = lsa_slam_save_dense_map_grid(this->Handle, &p, prefix.c_str());
    this->LastError = rc < 0 ? std::string("SaveDenseMapGrid: ") + lsa_slam_last_error(this->Handle) : std::string();
    return rc;
  }
  static lsa_dense_grid_params_t GridParams(const DenseGridParams& params)
  {
    lsa_dense_grid_params_t p;
    std::memset(&p, 0, sizeof(p));
    p.cell_leaves = params.cellLeaves; p.ground_radius = params.groundRadius; p.min_obstacle_voxels = params.minObstacleVoxels; p.min_frames = params.minFrames;
    p.min_height = params.minHeight; p.max_height = params.maxHeight; p.max_miss_ratio = params.maxMissRatio;
    p.use_window = params.useWindow ? 1 : 0;
    p.window[0] = params.xMin; p.window[1] = params.yMin; p.window[2] = params.xMax; p.window[3] = params.yMax;
    return p;
  }
  // float xyz per point of GetRegisteredFrame(), in its order: where the sensor stood when it measured the point
  std::vector<float> GetRegisteredFrameOrigins()
  {
    std::vector<float> out(3 * (static_cast<std::size_t>(1) << 19));
    int n = lsa_slam_get_registered_frame_origins(this->Handle, out.data(), static_cast<int>(out.size() / 3));
    out.resize(3 * static_cast<std::size_t>(std::max(n, 0)));
    this->LastError = n < 0 ? std::string("GetRegisteredFrameOrigins: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  // Rays: what the dense map holds along a line, answered on the device from the table as it stands (nothing is added to a
  // frame, nothing in the map changes).  A ray runs from an origin towards a target and `extend` metres past it (+inf: to
  // maxRange, the target only a direction), and stops at the first voxel that counts: seen in minFrames frames, misses <=
  // maxMissRatio * frames for a ratio >= 0, and -- useBefore 1 -- first seen before the ordinal `before`.  A DenseHit: status
  // (-1 no ray, 0 miss, 1 hit), the metres along the ray at which it enters and leaves the hit voxel, the voxel's kept point
  // projected on the ray (depth), the voxels visited, the voxel's key and source ordinal.
  struct DenseCastParams
  {
    double maxRange = 30., extend = 0., maxMissRatio = -1.;
    int minFrames = 1, useBefore = 0, before = 0;
    DenseCastParams() {}
  };
  struct DenseHit
  {
    std::uint64_t key;
    float entry, exit, depth;
    std::int32_t steps, source, status;
  };
  static lsa_dense_cast_params_t CastParams(const DenseCastParams& params)
  {
    lsa_dense_cast_params_t p;
    std::memset(&p, 0, sizeof(p));
    p.max_range = params.maxRange; p.extend = params.extend; p.max_miss_ratio = params.maxMissRatio;
    p.min_frames = params.minFrames; p.use_before = params.useBefore; p.before = params.before;
    return p;
  }
  // origins: xyz of one origin for all rays, or of one per ray; targets: xyz per ray
  std::vector<DenseHit> CastDenseMapRays(const std::vector<float>& origins, const std::vector<float>& targets, const DenseCastParams& params = DenseCastParams())
  {
    static_assert(sizeof(DenseHit) == sizeof(lsa_dense_hit_t), "DenseHit is lsa_dense_hit_t");
    const lsa_dense_cast_params_t p = CastParams(params);
    const int n = static_cast<int>(targets.size() / 3);
    std::vector<DenseHit> out(static_cast<std::size_t>(n));
    DenseHit none;
    const int rc = lsa_slam_cast_dense_map_rays(this->Handle, origins.data(), static_cast<int>(origins.size() / 3), targets.data(), n, &p,
                                                reinterpret_cast<lsa_dense_hit_t*>(n ? out.data() : &none), nullptr);
    if (rc < 0) out.clear();
    this->LastError = rc < 0 ? std::string("CastDenseMapRays: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  // a scan of the map as a spinning sensor of these ring elevations (radians) and nAzimuth columns would see it from the current
  // pose (or from `pose`, row-major 4x4): ring-major, column c at azimuth 2 pi c / nAzimuth; every ray runs to maxRange
  std::vector<DenseHit> RenderDenseMapScan(const std::vector<double>& elevations, int nAzimuth, DenseCastParams params = DenseCastParams(), const double* pose = nullptr)
  {
    params.extend = std::numeric_limits<double>::infinity();
    const lsa_dense_cast_params_t p = CastParams(params);
    const std::size_t n = elevations.size() * static_cast<std::size_t>(std::max(nAzimuth, 0));
    std::vector<DenseHit> out(std::max<std::size_t>(n, 1));
    const int rc = lsa_slam_render_dense_map_scan(this->Handle, pose, elevations.data(), static_cast<int>(elevations.size()), nAzimuth, &p,
                                                  reinterpret_cast<lsa_dense_hit_t*>(out.data()));
    out.resize(rc < 0 ? 0 : n);
    this->LastError = rc < 0 ? std::string("RenderDenseMapScan: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }
  // The current frame against the map: one label per point of GetRegisteredFrame(), in its order, from the ray of the point
  // (from where the sensor stood when it measured it) walked to `tolerance` metres behind the point (negative: one leaf):
  // DENSE_UNMAPPED nothing that counts lies on the ray -- the point is new to the map: the car that arrived --,
  // DENSE_CONSISTENT the ray meets the map at the point, DENSE_THROUGH_MAP it left a voxel that counts more than the tolerance
  // before the point, DENSE_NOT_JUDGED no ray or a point beyond maxRange.  automatic (the default): when this frame is in the
  // map itself, the map as it stood before it.  Two limits of a test by voxels: at tolerance 0 a point exactly on a voxel face
  // may end its walk one voxel short, and at grazing incidence far ground reads THROUGH_MAP at a small tolerance; UNMAPPED is
  // the robust label.  counts: the number of each label.
  enum DenseLabel : std::uint8_t { DENSE_NOT_JUDGED = 0, DENSE_CONSISTENT = 1, DENSE_UNMAPPED = 2, DENSE_THROUGH_MAP = 3 };
  std::vector<std::uint8_t> CompareFrameToDenseMap(long long counts[4] = nullptr, double tolerance = -1., DenseCastParams params = DenseCastParams(), bool automatic = true)
  {
    params.extend = tolerance < 0. ? this->GetDenseMapLeafSize() : tolerance;
    lsa_dense_cast_params_t p = CastParams(params);
    if (automatic) p.use_before = 2;
    std::vector<std::uint8_t> out(static_cast<std::size_t>(1) << 19);
    long long c[4] = {0, 0, 0, 0};
    int n = lsa_slam_compare_frame_to_dense_map(this->Handle, &p, out.data(), static_cast<int>(out.size()), c);
    // a frame of more points than that (several device frames in one AddFrames call): the call refuses before it touches
    // anything, and is asked again with more room
    while (n == LSA_E_CAPACITY && out.size() < (static_cast<std::size_t>(1) << 28))
    {
      out.resize(out.size() * 4);
      n = lsa_slam_compare_frame_to_dense_map(this->Handle, &p, out.data(), static_cast<int>(out.size()), c);
    }
    out.resize(static_cast<std::size_t>(std::max(n, 0)));
    if (counts)
      for (int l = 0; l < 4; ++l) counts[l] = n < 0 ? 0 : c[l];
    this->LastError = n < 0 ? std::string("CompareFrameToDenseMap: ") + lsa_slam_last_error(this->Handle) : std::string();
    return out;
  }

  // ---- keypoint extractor parameters (SpinningSensorKeypointExtractor.h:44-70); one extractor (device 0)
  LSA_SLAM_PARAM(NeighborWidth, int)
  LSA_SLAM_PARAM(MinDistanceToSensor, float)
  LSA_SLAM_PARAM(MinBeamSurfaceAngle, float)
  LSA_SLAM_PARAM(PlaneSinAngleThreshold, float)
  LSA_SLAM_PARAM(EdgeSinAngleThreshold, float)
  LSA_SLAM_PARAM(EdgeDepthGapThreshold, float)
  LSA_SLAM_PARAM(EdgeSaliencyThreshold, float)
  LSA_SLAM_PARAM(EdgeIntensityGapThreshold, float)
  LSA_SLAM_PARAM(AzimuthalResolution, float)

  // generic access by the reference's setter name (without "Set")
  void SetParam(const std::string& name, double v)
  {
    if (lsa_slam_set_param(this->Handle, name.c_str(), v) != LSA_OK) throw std::invalid_argument("LidarSlam::Slam: unknown parameter " + name);
  }
  double GetParam(const std::string& name) const
  {
    double v = 0.;
    if (lsa_slam_get_param(this->Handle, name.c_str(), &v) != LSA_OK) throw std::invalid_argument("LidarSlam::Slam: unknown parameter " + name);
    return v;
  }
  lsa_slam* GetHandle() { return this->Handle; }

private:
  // one staging buffer per Slam, kept between calls (the wrappers call the getters every frame: no 16 MB allocation per call)
  template <typename F> PointCloud::Ptr Fetch(F f, const std::string& frame)
  {
    PointCloud::Ptr pc(new PointCloud);
    if (this->Staging.size() < (1u << 19)) this->Staging.resize(1u << 19);
    int n = f(this->Staging.data(), static_cast<int>(this->Staging.size()));
    while (n >= static_cast<int>(this->Staging.size()) && this->Staging.size() < (1u << 26))
    {
      this->Staging.resize(this->Staging.size() * 4);  // it may have been cut short: once more with room
      n = f(this->Staging.data(), static_cast<int>(this->Staging.size()));
    }
    if (n < 0) n = 0;
    n = std::min<int>(n, static_cast<int>(this->Staging.size()));
    pc->points.resize(n);
    if (n > 0) std::memcpy(static_cast<void*>(pc->points.data()), this->Staging.data(), static_cast<std::size_t>(n) * sizeof(lsa_point_t));
    pc->header.stamp = this->CurrentStamp;
    pc->header.frame_id = frame;
    return pc;
  }

  void WarnOnce(const char* what, const char* why) const
  {
    if (this->Warned.insert(what).second) std::fprintf(stderr, "\033[1;33m[WARNING] LidarSlam::Slam::%s: %s\033[0m\n", what, why);
  }
  void NotSupported(const char* what, const char* why) const { this->WarnOnce(what, why); }
  void ReportMapIO(const char* what, const char* verb, const std::string& prefix, int rc) const
  {
    // GetLastError() speaks of the last call: a save or load that went well clears what an earlier one left
    this->LastError = rc < 0 ? std::string(what) + ": " + lsa_slam_last_error(this->Handle) : std::string();
    if (!this->Warned.insert(what).second) return;
    static const char* const names[3] = {"edges", "planes", "blobs"};
    int counts[3] = {-1, -1, -1};
    lsa_slam_map_io_counts(this->Handle, counts);
    std::string line;
    for (int k = 0; k < 3; ++k)
      if (counts[k] >= 0) line += " " + prefix + names[k] + ".pcd (" + std::to_string(counts[k]) + " points)";
    if (rc < 0) line = " failed: " + this->LastError;
    else if (line.empty()) line = " no file";
    std::fprintf(stderr, "LidarSlam::Slam::%s: keypoint maps %s%s\n", what, verb, line.c_str());
  }

  lsa_slam* Handle = nullptr;
  mutable std::set<std::string> Warned;
  std::vector<lsa_point_t> Staging;  // Fetch
  std::map<std::uint8_t, KeypointExtractorPtr> KeyPointsExtractors;
  std::uint64_t CurrentStamp = 0;
  std::string WorldFrameId = "world", BaseFrameId = "base";
  mutable std::string LastError;  // mutable: SaveMapsToPCD is const in the reference and reports its failure here
  int Verbosity = 0;
};

#undef LSA_SLAM_PARAM
#undef LSA_SLAM_ENUM_PARAM

}  // namespace LidarSlam
