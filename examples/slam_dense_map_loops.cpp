// The map you came for survives the loop closure: the forward-and-back drive of slam_close_loops.cpp mapped with the dense
// point-cloud map on and SetDenseMapOnTrajectory(1), so that CloseLoops -- which applies the optimized trajectory -- re-projects
// the dense map on the device instead of clearing it: one point per voxel, moved by the correction of the frame that measured
// it.  Written against the reference's C++ API and linked with liblidarslam_amd.so.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_dense_map_loops.cpp
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_dense_map_loops      (one command line)
//   ./slam_dense_map_loops <directory> [model=16] [forward=12] [leaf=0.2]
// writes <directory>/dense_before.pcd and <directory>/dense.pcd (after the loops are closed); prints "# before <voxels>",
// "# loops <reports> <edges>", "# after <voxels> <dropped> <reprojections> <clears>" and "# sources <voxels> <oldest> <newest>"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
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
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: %s <directory> [model] [forward] [leaf]\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int model = argc > 2 ? std::atoi(argv[2]) : 16;
  const int forward = argc > 3 ? std::atoi(argv[3]) : 12;
  const double leaf = argc > 4 ? std::atof(argv[4]) : 0.2;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetLoggingTimeout(-1.);  // every pose and its keypoints are logged
    slam.SetDenseMapLeafSize(leaf);
    slam.SetDenseMap(1);              // every registered frame
    slam.SetDenseMapOnTrajectory(1);  // an applied trajectory re-projects the map instead of clearing it
    std::uint64_t firstStamp = 0, period = 0;
    int seq = 0;
    for (int f = 0; f < forward; ++f, ++seq) slam.AddFrame(Frame(model, f, seq, &firstStamp, &period));
    for (int f = forward - 2; f >= 0; --f, ++seq) slam.AddFrame(Frame(model, f, seq, &firstStamp, &period));
    const int before = slam.SaveDenseMapToPCD(dir + "/dense_before.pcd", LidarSlam::PCDFormat::BINARY, 1);
    if (before < 0)
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    std::printf("# before %d\n", before);

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
    pgo.apply = 1;
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
    int edges = 0;
    for (const LidarSlam::Slam::LoopReport& r : reports) edges += r.edge >= 0 ? 1 : 0;
    std::printf("# loops %d %d\n", (int)reports.size(), edges);

    const int after = slam.SaveDenseMapToPCD(dir + "/dense.pcd", LidarSlam::PCDFormat::BINARY, 1);
    if (after < 0)
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    std::printf("# after %d %d %d %d\n", after, (int)slam.GetParam("DenseMapDropped"), (int)slam.GetParam("DenseMapReprojections"), (int)slam.GetParam("DenseMapClears"));
    const std::vector<int> sources = slam.GetDenseMapSources(1);
    if (!sources.empty())
      std::printf("# sources %d %d %d\n", (int)sources.size(), *std::min_element(sources.begin(), sources.end()), *std::max_element(sources.begin(), sources.end()));
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
