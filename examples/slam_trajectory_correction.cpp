// A trajectory corrected after the fact, brought back into the library: written against the reference's C++ API and linked
// with liblidarslam_amd.so.  A Slam maps N frames with the keypoint log on (SetLoggingTimeout(-1)); the logged trajectory
// is bent the way an optimizer -- g2o, GTSAM, Ceres, GPS, control points -- would correct a drift; SetTrajectoryAndRebuildMaps
// replaces the poses and rebuilds the maps from the logged keypoints under them; two more frames go on in the rebuilt maps.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_trajectory_correction.cpp \
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_trajectory_correction
//   ./slam_trajectory_correction [model=16] [mapped=8]
// prints "frame x y z" of the corrected poses and of the two that follow, "# maps <edges> <planes>" before and after the
// rebuild, "# logged <frames> <planes of frame 0> <bytes>"
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char** argv)
{
  const int model = argc > 1 ? std::atoi(argv[1]) : 16;
  const int mapped = argc > 2 ? std::atoi(argv[2]) : 8;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetLoggingTimeout(-1.);  // every pose and its keypoints are logged
    slam.SetLoggingStorage(LidarSlam::PointCloudStorageType::PCL_CLOUD);
    for (int f = 0; f < mapped; ++f) slam.AddFrame(Frame(model, f));
    std::printf("# maps %d %d\n", (int)slam.GetMap(LidarSlam::EDGE)->size(), (int)slam.GetMap(LidarSlam::PLANE)->size());
    std::printf("# logged %d %d %.0f\n", (int)slam.GetTrajectory().size(), (int)slam.GetLoggedKeypoints(LidarSlam::PLANE, 0)->size(), slam.GetParam("LoggedKeypointsBytes"));
    // the correction: pose i turned by 0.002 i rad about z and moved by 0.05 i m, P'[i] = C[i] P[i]
    std::vector<LidarSlam::Transform> poses = slam.GetTrajectory();
    for (std::size_t i = 0; i < poses.size(); ++i)
    {
      const double a = 0.002 * i, c = std::cos(a), s = std::sin(a), tx = 0.05 * i * 0.6, ty = 0.05 * i * 0.8;
      std::array<double, 16>& m = poses[i].matrix;
      for (int col = 0; col < 4; ++col)
      {
        const double r0 = m[col], r1 = m[4 + col];
        m[col] = c * r0 - s * r1 + (col == 3 ? tx : 0.);
        m[4 + col] = s * r0 + c * r1 + (col == 3 ? ty : 0.);
      }
    }
    slam.SetTrajectoryAndRebuildMaps(poses);
    if (!slam.GetLastError().empty())
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    int f = 0;
    for (const LidarSlam::Transform& T : slam.GetTrajectory()) std::printf("%d %.12f %.12f %.12f\n", f++, T.x(), T.y(), T.z());
    std::printf("# maps %d %d\n", (int)slam.GetMap(LidarSlam::EDGE)->size(), (int)slam.GetMap(LidarSlam::PLANE)->size());
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
