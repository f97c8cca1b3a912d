// Every loop closure of a logged drive found and closed in one call, written against the reference's C++ API and linked with
// liblidarslam_amd.so.  A Slam maps N frames forward with the keypoint log on (SetLoggingTimeout(-1)) and then the same clouds
// in reverse order: the vehicle backs up over its own track, so every frame of the way back revisits a place.  CloseLoops
// detects the revisits of the whole log on the device, registers every candidate, solves the pose graph of the logged odometry
// and these edges under Tukey's loss -- an edge that contradicts the rest is discounted, not obeyed -- and rebuilds the maps
// under the result; two more frames are then added on top.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_close_loops.cpp
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_close_loops      (one command line)
//   ./slam_close_loops [model=16] [forward=12]
// prints "# loop <query> <frame> <descriptor distance> <yaw> <status> <iterations> <position error> <edge> <chi2> <weight>"
// for every candidate, "# solve <termination> <LM iterations> <PCG iterations>", "# cost <initial> <final>", "# last x y z" (the
// optimized last pose's position), and "# frame x y z" for each of the two frames added afterwards
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <vector>
#include "LidarSlam/Slam.h"

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

    // every third frame of the way back asks where it has been before
    LidarSlam::Slam::LoopDetectionParameters detect = LidarSlam::Slam::DefaultLoopDetectionParameters();
    detect.search.min_travelled = 2.;
    detect.search.max_distance = 0.;
    detect.search.exclusion_half_window = 2;
    detect.first_query = forward + 2;
    detect.query_stride = 3;
    detect.per_query = 1;
    LidarSlam::Slam::LoopClosureParameters loop = LidarSlam::Slam::DefaultLoopClosureParameters();
    loop.revisited_half_window = 2;
    LidarSlam::Slam::PoseGraphParameters pgo = LidarSlam::Slam::DefaultPoseGraphParameters();
    pgo.apply = 1;  // the maps are rebuilt under the optimized trajectory
    LidarSlam::Slam::RobustParameters robust = LidarSlam::Slam::DefaultRobustParameters();
    robust.edge_loss = LSA_PGO_LOSS_TUKEY;
    robust.edge_scale = 3.;
    LidarSlam::Slam::PoseGraphSummary summary;
    std::vector<LidarSlam::Slam::LoopReport> reports;
    const std::vector<LidarSlam::Transform> optimized = slam.CloseLoops(detect, loop, pgo, robust, &summary, &reports);
    if (optimized.empty())
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 2;
    }
    for (const LidarSlam::Slam::LoopReport& r : reports)
      std::printf("# loop %d %d %.9g %.12f %d %d %.9g %d %.9g %.9g\n", r.query, r.frame, r.distance, r.yaw, r.status, r.iterations, r.position_error, r.edge, r.chi2, r.weight);
    std::printf("# solve %d %d %d\n", summary.termination, summary.iterations, summary.pcg_iterations);
    std::printf("# cost %.9g %.9g\n", summary.initial_cost, summary.final_cost);
    std::printf("# last %.12f %.12f %.12f\n", optimized.back().matrix[3], optimized.back().matrix[7], optimized.back().matrix[11]);
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
