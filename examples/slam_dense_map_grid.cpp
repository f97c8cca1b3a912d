// A map a planner can take: a short synthetic drive mapped with the dense point-cloud map and free-space carving on, then
// rasterised on the device into the 2-D occupancy grid of nav_msgs/OccupancyGrid -- occupied, free, unknown -- with the
// ground height under it: the whole plan, and the local costmap around the vehicle.
// Written against the reference's C++ API and linked with liblidarslam_amd.so.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_dense_map_grid.cpp \
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_dense_map_grid
//   ./slam_dense_map_grid <directory> [model=16] [frames=8] [leaf=0.2] [half_extent=10]
// writes <directory>/plan.pgm, plan.yaml (the whole map) and local.pgm, local.yaml (the window around the last pose) for
// map_server; prints "# plan <width> <height> <occupied> <free> <unknown>" and "# local ..." likewise
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

static void Report(const char* name, const LidarSlam::Slam::DenseGrid& grid)
{
  long long count[3] = {0, 0, 0};
  for (const std::int8_t s : grid.states) count[s == 100 ? 0 : (s == 0 ? 1 : 2)]++;
  std::printf("# %s %d %d %lld %lld %lld\n", name, grid.width, grid.height, count[0], count[1], count[2]);
}

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: %s <directory> [model] [frames] [leaf] [half_extent]\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  const int model = argc > 2 ? std::atoi(argv[2]) : 16;
  const int frames = argc > 3 ? std::atoi(argv[3]) : 8;
  const double leaf = argc > 4 ? std::atof(argv[4]) : 0.2;
  const double halfExtent = argc > 5 ? std::atof(argv[5]) : 10.;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetDenseMapLeafSize(leaf);
    slam.SetDenseMap(1);  // every registered frame
    slam.SetDenseMapCarve(1);
    for (int f = 0; f < frames; ++f) slam.AddFrame(Frame(model, f));
    // what was seen at least as often as seen through; cells of two voxels, the ground from two cells around
    LidarSlam::Slam::DenseGridParams params;
    params.maxMissRatio = 1.0;
    const LidarSlam::Slam::DenseGrid plan = slam.GetDenseMapGrid(params);
    const LidarSlam::Slam::DenseGrid local = slam.GetDenseMapGridAround(halfExtent, params);
    if (!slam.GetLastError().empty() || plan.states.empty() || local.states.empty())
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    LidarSlam::Slam::DenseGridParams window = params;
    window.useWindow = true;
    // the window of exactly those cells again, from half a voxel inside its first cell to half a voxel inside its last
    const double inside = 0.5 * local.resolution / params.cellLeaves;
    window.xMin = local.origin_x + inside;
    window.yMin = local.origin_y + inside;
    window.xMax = local.origin_x + local.resolution * local.width - inside;
    window.yMax = local.origin_y + local.resolution * local.height - inside;
    if (slam.SaveDenseMapGrid(dir + "/plan", params) != static_cast<long long>(plan.states.size()) ||
        slam.SaveDenseMapGrid(dir + "/local", window) != static_cast<long long>(local.states.size()))
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    Report("plan", plan);
    Report("local", local);
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
