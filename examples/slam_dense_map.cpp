// The map you came for: a short synthetic drive mapped with the dense point-cloud map on, saved as PCD files -- every voxel,
// and only the voxels seen in three frames or more --, written against the reference's C++ API and linked with
// liblidarslam_amd.so.  No registered frame leaves the device on the way.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_dense_map.cpp \
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_dense_map
//   ./slam_dense_map <directory> [model=16] [frames=8] [leaf=0.2] [format=1]
// writes <directory>/dense.pcd (minFrames 1) and <directory>/dense_3.pcd (minFrames 3); prints "# dense <all> <three frames>"
#include <cstdio>
#include <cstdlib>
#include <string>
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
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: %s <directory> [model] [frames] [leaf] [format]\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int model = argc > 2 ? std::atoi(argv[2]) : 16;
  const int frames = argc > 3 ? std::atoi(argv[3]) : 8;
  const double leaf = argc > 4 ? std::atof(argv[4]) : 0.2;
  const LidarSlam::PCDFormat format = static_cast<LidarSlam::PCDFormat>(argc > 5 ? std::atoi(argv[5]) : 1);
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetDenseMapLeafSize(leaf);
    slam.SetDenseMap(1);  // every registered frame
    for (int f = 0; f < frames; ++f) slam.AddFrame(Frame(model, f));
    const int all = slam.SaveDenseMapToPCD(dir + "/dense.pcd", format, 1);
    const int seen3 = all < 0 ? all : slam.SaveDenseMapToPCD(dir + "/dense_3.pcd", format, 3);
    if (all < 0 || seen3 < 0)
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    std::printf("# dense %d %d\n", all, seen3);
    std::printf("# fetched %d %d\n", (int)slam.GetDenseMap(1)->size(), (int)slam.GetDenseMap(3)->size());
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
