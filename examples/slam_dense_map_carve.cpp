// What moved away leaves the map: a short synthetic drive mapped with the dense point-cloud map and free-space carving on --
// every inserted point's ray, from where the sensor stood to shortly before the point, is walked through the voxel grid on the
// device, and a voxel seen through more often than seen is left out of a filtered export and removed by a prune.  Written
// against the reference's C++ API and linked with liblidarslam_amd.so.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_dense_map_carve.cpp \
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_dense_map_carve
//   ./slam_dense_map_carve <directory> [model=16] [frames=8] [leaf=0.2] [format=1] [stride=1]
// writes <directory>/dense_all.pcd (every voxel), dense_seen.pcd (misses <= frames) and dense_pruned.pcd (the map after
// PruneDenseMap(1, 1.0)); prints "# carve <all> <filtered> <after the prune>" and "# pruned <removed> <rays>"
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
    std::fprintf(stderr, "usage: %s <directory> [model] [frames] [leaf] [format] [stride]\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int model = argc > 2 ? std::atoi(argv[2]) : 16;
  const int frames = argc > 3 ? std::atoi(argv[3]) : 8;
  const double leaf = argc > 4 ? std::atof(argv[4]) : 0.2;
  const LidarSlam::PCDFormat format = static_cast<LidarSlam::PCDFormat>(argc > 5 ? std::atoi(argv[5]) : 1);
  const int stride = argc > 6 ? std::atoi(argv[6]) : 1;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetDenseMapLeafSize(leaf);
    slam.SetDenseMap(1);  // every registered frame
    slam.SetDenseMapCarve(1);
    slam.SetDenseMapCarveStride(stride);
    for (int f = 0; f < frames; ++f) slam.AddFrame(Frame(model, f));
    const int all = slam.SaveDenseMapToPCD(dir + "/dense_all.pcd", format, 1);
    const int seen = all < 0 ? all : slam.SaveDenseMapToPCD(dir + "/dense_seen.pcd", format, 1, 1.0);
    const long long removed = seen < 0 ? seen : slam.PruneDenseMap(1, 1.0);
    const int left = removed < 0 ? -1 : slam.SaveDenseMapToPCD(dir + "/dense_pruned.pcd", format, 1);
    if (all < 0 || seen < 0 || removed < 0 || left < 0)
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    std::printf("# carve %d %d %d\n", all, seen, left);
    std::printf("# pruned %lld %.0f\n", removed, slam.GetParam("DenseMapRays"));
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
