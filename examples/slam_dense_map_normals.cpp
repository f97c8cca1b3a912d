// A map a mesher can take: a short synthetic drive mapped with the dense point-cloud map and free-space carving on, saved
// with one normal per point -- the eigenvector of the smallest eigenvalue of the covariance of the kept points within two
// voxels, computed on the device from the voxel table and turned towards where the sensor stood when it measured the point.
// Written against the reference's C++ API and linked with liblidarslam_amd.so.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_dense_map_normals.cpp \
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_dense_map_normals
//   ./slam_dense_map_normals <directory> [model=16] [frames=8] [leaf=0.2] [format=1]
// writes <directory>/dense_normals.pcd (x y z time intensity laser_id device_id label normal_x normal_y normal_z curvature) of the
// voxels with misses <= frames; prints "# normals <voxels> <voxels without a normal>"
#include <cmath>
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
    slam.SetDenseMapCarve(1);
    for (int f = 0; f < frames; ++f) slam.AddFrame(Frame(model, f));
    // what was seen at least as often as seen through, radius 2 leaves, 5 neighbours at least, oriented
    const int saved = slam.SaveDenseMapWithNormalsToPCD(dir + "/dense_normals.pcd", format, 1, 1.0, 2, 5, true);
    const std::vector<LidarSlam::Slam::DenseNormal> normals = slam.GetDenseMapNormals(1, 1.0, 2, 5, true);
    if (saved < 0 || static_cast<int>(normals.size()) != saved)
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    int without = 0;
    for (const LidarSlam::Slam::DenseNormal& n : normals) without += std::isnan(n.normal_x) ? 1 : 0;
    std::printf("# normals %d %d\n", saved, without);
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
