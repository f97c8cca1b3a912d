// Pose-graph optimization with GPS positions, written against the reference's C++ API and linked with liblidarslam_amd.so.
// A Slam maps N frames forward with the keypoint log on (SetLoggingTimeout(-1)) and then the same clouds in reverse order.  A
// GPS track is made from the logged poses: the antenna sits behind a lever arm on the vehicle, the GPS frame is a known world
// transform away from the SLAM's, and the track is bent smoothly by up to 0.2 m, as drift would.  RunPoseGraphOptimization
// matches fixes and poses by time, solves the graph of the logged odometry and the position priors on the device, rebuilds the
// maps under the result and returns the calibration: the first pose in the GPS frame.  Two more frames are then added on top.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_gps_pose_graph.cpp
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_gps_pose_graph      (one command line)
//   ./slam_gps_pose_graph [model=16] [forward=12]
// prints "# gps <fixes>", "# solve <termination> <LM iterations> <PCG iterations>", "# cost <initial> <final>", "# last x y z" (the
// optimized last pose's position), "# calibration x y z" (the first pose's position in the GPS frame) and "# frame x y z" for each
// of the two frames added afterwards
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>
#include "LidarSlam/Slam.h"

using Matrix = std::array<double, 16>;  // row-major 4x4

static Matrix Mul(const Matrix& a, const Matrix& b)
{
  Matrix c{};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k) c[4 * i + j] += a[4 * i + k] * b[4 * k + j];
  return c;
}
static Matrix RigidInverse(const Matrix& a)
{
  Matrix c{};
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j) c[4 * i + j] = a[4 * j + i];
    c[4 * i + 3] = -(a[i] * a[3] + a[4 + i] * a[7] + a[8 + i] * a[11]);
  }
  c[15] = 1.;
  return c;
}

static LidarSlam::Slam::PointCloud::Ptr Frame(int model, int cloud, int seq, std::uint64_t* firstStamp, std::uint64_t* period)
{
  LidarSlam::Slam::PointCloud::Ptr pc(new LidarSlam::Slam::PointCloud);
  pc->points.resize(1 << 19);
  std::uint64_t stamp = 0;
  const int n = lsa_synth_frame(model, 1000, cloud, reinterpret_cast<lsa_point_t*>(pc->points.data()), (int)pc->points.size(), &stamp);
  pc->points.resize(n > 0 ? n : 0);
  if (seq == 0) *firstStamp = stamp;
  if (seq == 1) *period = stamp - *firstStamp;
  pc->header.stamp = *firstStamp + seq * *period;  // the clouds come again, the clock goes on
  pc->header.seq = seq;
  return pc;
}

int main(int argc, char** argv)
{
  const int model = argc > 1 ? std::atoi(argv[1]) : 16;
  const int forward = argc > 2 ? std::atoi(argv[2]) : 12;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetLoggingTimeout(-1.);  // every pose and its keypoints are logged
    std::uint64_t firstStamp = 0, period = 0;
    int seq = 0;
    for (int f = 0; f < forward; ++f, ++seq) slam.AddFrame(Frame(model, f, seq, &firstStamp, &period));
    for (int f = forward - 2; f >= 0; --f, ++seq) slam.AddFrame(Frame(model, f, seq, &firstStamp, &period));

    // the GPS track: the antenna of every logged pose seen from the GPS frame, bent smoothly
    const Matrix world = LidarSlam::Transform(100., -50., 10., 0.02, -0.03, 0.8).matrix;
    const Matrix antenna = LidarSlam::Transform(0.4, -0.3, 1.2, 0.1, -0.2, 0.3).matrix;  // the antenna's pose in BASE
    const std::vector<LidarSlam::Transform> logged = slam.GetTrajectory();
    const int n = static_cast<int>(logged.size());
    std::vector<LidarSlam::Transform> gps;
    std::vector<std::array<double, 9>> gpsCovariances;
    for (int i = 0; i < n; ++i)
    {
      const Matrix at = Mul(Mul(world, logged[i].matrix), antenna);
      const double bend = 0.2 * std::sin(3.141592653589793 * i / (n - 1));
      LidarSlam::Transform fix;
      fix.x() = at[3];
      fix.y() = at[7] + 0.8 * bend;
      fix.z() = at[11] + 0.6 * bend;
      fix.time = logged[i].time;
      gps.push_back(fix);
      gpsCovariances.push_back({{9e-4, 0., 0., 0., 9e-4, 0., 0., 0., 9e-4}});  // 0.03 m
    }
    std::printf("# gps %d\n", n);
    // the reference's calibration argument: its inverse is the offset behind which the fixes are expected
    Matrix gpsToSensor = RigidInverse(antenna);
    LidarSlam::Slam::PoseGraphParameters pgo = LidarSlam::Slam::DefaultPoseGraphParameters();
    pgo.odometry_information = 1;  // the inverse of the logged covariances, the reference's rule
    pgo.apply = 1;                 // the maps are rebuilt under the optimized trajectory
    LidarSlam::Slam::PoseGraphSummary summary;
    const std::vector<LidarSlam::Transform> optimized = slam.RunPoseGraphOptimization(gps, gpsCovariances, gpsToSensor, pgo, 0., &summary);
    if (optimized.empty())
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 5;
    }
    std::printf("# solve %d %d %d\n", summary.termination, summary.iterations, summary.pcg_iterations);
    std::printf("# cost %.9g %.9g\n", summary.initial_cost, summary.final_cost);
    std::printf("# last %.12f %.12f %.12f\n", optimized.back().matrix[3], optimized.back().matrix[7], optimized.back().matrix[11]);
    std::printf("# calibration %.12f %.12f %.12f\n", gpsToSensor[3], gpsToSensor[7], gpsToSensor[11]);
    for (int f = 1; f <= 2; ++f, ++seq)
    {
      slam.AddFrame(Frame(model, f, seq, &firstStamp, &period));
      const std::array<double, 16> T = slam.GetWorldTransform().matrix;
      std::printf("# frame %.12f %.12f %.12f\n", T[3], T[7], T[11]);
    }
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
