// A loop closure from the keypoint log, written against the reference's C++ API and linked with liblidarslam_amd.so.  A Slam
// maps N frames with the keypoint log on (SetLoggingTimeout(-1)); FindLoopClosureCandidate names an earlier logged frame near
// the last but two; RegisterLoggedFrames registers that query frame against the logged keypoints around the candidate (on the
// device: nothing but the result comes back); the correction it finds is spread over the poses between the two, the way a
// pose-graph optimizer with this one loop edge and equal weights on the odometry edges would; SetTrajectoryAndRebuildMaps
// brings the corrected trajectory back and rebuilds the maps; two more frames go on in the rebuilt maps.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_loop_closure.cpp
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_loop_closure      (one command line)
//   ./slam_loop_closure [model=16] [mapped=12]
// prints "# candidate <query> <revisited>", "# registered <status> <iterations> <target edges> <target planes> <query edges>
// <query planes>", "# world x y z", "# relative x y z", "# errors <position [m]> <orientation [deg]>", then "frame x y z" of
// the corrected poses and of the two that follow
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>
#include "LidarSlam/Slam.h"

static LidarSlam::Slam::PointCloud::Ptr Frame(int model, int f)
{
  LidarSlam::Slam::PointCloud::Ptr pc(new LidarSlam::Slam::PointCloud);
  pc->points.resize(1 << 19);
  std::uint64_t stamp = 0;
  const int n = lsa_synth_frame(model, 1000, f, reinterpret_cast<lsa_point_t*>(pc->points.data()), (int)pc->points.size(), &stamp);
  pc->points.resize(n > 0 ? n : 0);
  pc->header.stamp = stamp;
  pc->header.seq = f;
  return pc;
}

using Mat = std::array<double, 16>;  // row-major 4x4, rigid

static Mat Mul(const Mat& a, const Mat& b)
{
  Mat r{};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k) r[4 * i + j] += a[4 * i + k] * b[4 * k + j];
  return r;
}
static Mat Inv(const Mat& a)
{
  Mat r{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) r[4 * i + j] = a[4 * j + i];
  for (int i = 0; i < 3; ++i) r[4 * i + 3] = -(r[4 * i] * a[3] + r[4 * i + 1] * a[7] + r[4 * i + 2] * a[11]);
  return r;
}
// the share `s` of a small rigid correction: its translation times s, its rotation about the same axis by s times its angle
static Mat Share(const Mat& c, double s)
{
  const double w[3] = {(c[9] - c[6]) / 2, (c[2] - c[8]) / 2, (c[4] - c[1]) / 2};  // axis * sin(angle)
  const double sine = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]), cosine = (c[0] + c[5] + c[10] - 1) / 2;
  const double angle = std::atan2(sine, cosine);
  Mat r{{1, 0, 0, s * c[3], 0, 1, 0, s * c[7], 0, 0, 1, s * c[11], 0, 0, 0, 1}};
  if (sine < 1e-15) return r;
  const double u[3] = {w[0] / sine, w[1] / sine, w[2] / sine}, a = s * angle, ca = std::cos(a), sa = std::sin(a);
  const double K[9] = {0, -u[2], u[1], u[2], 0, -u[0], -u[1], u[0], 0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
    {
      double kk = 0;
      for (int k = 0; k < 3; ++k) kk += K[3 * i + k] * K[3 * k + j];
      r[4 * i + j] = (i == j ? 1. : 0.) + sa * K[3 * i + j] + (1 - ca) * kk;
    }
  return r;
}

int main(int argc, char** argv)
{
  const int model = argc > 1 ? std::atoi(argv[1]) : 16;
  const int mapped = argc > 2 ? std::atoi(argv[2]) : 12;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetLoggingTimeout(-1.);  // every pose and its keypoints are logged
    for (int f = 0; f < mapped; ++f) slam.AddFrame(Frame(model, f));

    // a place seen before: at least 2.2 m back along the trajectory, within 4 m of where the query frame was taken
    const int query = mapped - 3;
    const int revisited = slam.FindLoopClosureCandidate(query, 2.2, 4.0);
    std::printf("# candidate %d %d\n", query, revisited);
    if (revisited < 0) return 2;

    LidarSlam::Slam::LoopClosureParameters params = LidarSlam::Slam::DefaultLoopClosureParameters();
    params.revisited_half_window = 2;
    const LidarSlam::Slam::LoopClosureRegistration reg = slam.RegisterLoggedFrames(query, revisited, params);
    if (reg.status < 0)
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    std::printf("# registered %d %d %lld %lld %lld %lld\n", reg.status, reg.iterations, (long long)reg.target_points[LidarSlam::EDGE], (long long)reg.target_points[LidarSlam::PLANE],
                (long long)reg.query_points[LidarSlam::EDGE], (long long)reg.query_points[LidarSlam::PLANE]);
    std::printf("# world %.12f %.12f %.12f\n", reg.world[3], reg.world[7], reg.world[11]);
    std::printf("# relative %.12f %.12f %.12f\n", reg.relative[3], reg.relative[7], reg.relative[11]);
    std::printf("# errors %.9f %.9f\n", reg.position_error, reg.orientation_error);

    // the correction of the query pose, C = registered * inv(logged), spread over the poses between the two: pose i gets the
    // share (i - revisited) / (query - revisited) of it, the poses after the query all of it
    std::vector<LidarSlam::Transform> poses = slam.GetTrajectory();
    Mat world;
    for (int i = 0; i < 16; ++i) world[i] = reg.world[i];
    const Mat correction = Mul(world, Inv(poses[query].matrix));
    for (int i = revisited + 1; i < (int)poses.size(); ++i)
    {
      const double share = i >= query ? 1. : double(i - revisited) / double(query - revisited);
      poses[i].matrix = Mul(Share(correction, share), poses[i].matrix);
    }
    slam.SetTrajectoryAndRebuildMaps(poses);
    if (!slam.GetLastError().empty())
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    int f = 0;
    for (const LidarSlam::Transform& T : slam.GetTrajectory()) std::printf("%d %.12f %.12f %.12f\n", f++, T.x(), T.y(), T.z());
    for (f = mapped; f < mapped + 2; ++f)
    {
      slam.AddFrame(Frame(model, f));
      const LidarSlam::Transform T = slam.GetWorldTransform();
      std::printf("%d %.12f %.12f %.12f\n", f, T.x(), T.y(), T.z());
    }
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
