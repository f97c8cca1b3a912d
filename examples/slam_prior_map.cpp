// Map once, localize later: the reference's production use of SaveMapsToPCD / LoadMapsFromPCD, written against its C++
// API and linked with liblidarslam_amd.so.  A first Slam maps N frames and saves its keypoint maps; a fresh Slam with
// MapUpdate = NONE loads them, is told where it is, and localizes the following frames inside the saved map.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_prior_map.cpp \
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_prior_map
//   ./slam_prior_map <prefix> [model=16] [mapped=6] [localized=4] [format=2]
// prints "frame x y z" of every localized pose, then "# maps <edges> <planes>" of the loaded maps
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
    std::fprintf(stderr, "usage: %s <prefix> [model] [mapped] [localized] [format]\n", argv[0]);
    return 2;
  }
  const std::string prefix = argv[1];
  const int model = argc > 2 ? std::atoi(argv[2]) : 16;
  const int mapped = argc > 3 ? std::atoi(argv[3]) : 6;
  const int localized = argc > 4 ? std::atoi(argv[4]) : 4;
  const LidarSlam::PCDFormat format = static_cast<LidarSlam::PCDFormat>(argc > 5 ? std::atoi(argv[5]) : 2);
  try
  {
    LidarSlam::Transform where;
    {
      LidarSlam::Slam mapper;
      mapper.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
      mapper.SetVoxelGridMinFramesPerVoxel(1);
      for (int f = 0; f < mapped; ++f) mapper.AddFrame(Frame(model, f));
      where = mapper.GetWorldTransform();
      mapper.SaveMapsToPCD(prefix, format, false);
      if (!mapper.GetLastError().empty())
      {
        std::fprintf(stderr, "%s\n", mapper.GetLastError().c_str());
        return 3;
      }
    }
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetVoxelGridMinFramesPerVoxel(1);
    slam.SetMapUpdate(LidarSlam::MappingMode::NONE);  // the loaded points are fixed, nothing is added
    slam.LoadMapsFromPCD(prefix);
    if (!slam.GetLastError().empty())
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    slam.SetWorldTransformFromGuess(where);
    for (int f = mapped; f < mapped + localized; ++f)
    {
      slam.AddFrame(Frame(model, f));
      const LidarSlam::Transform T = slam.GetWorldTransform();
      std::printf("%d %.12f %.12f %.12f\n", f, T.x(), T.y(), T.z());
    }
    std::printf("# maps %d %d\n", (int)slam.GetMap(LidarSlam::EDGE, false)->size(), (int)slam.GetMap(LidarSlam::PLANE, false)->size());
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
