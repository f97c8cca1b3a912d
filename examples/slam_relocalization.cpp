// Map once, localize later WITHOUT being told where: place recognition against the saved maps, written against the reference's
// C++ API and linked with liblidarslam_amd.so.  A first Slam maps N frames and saves its keypoint maps and the positions it
// drove through.  A fresh Slam with MapUpdate = NONE loads the maps and is switched on somewhere inside them, the base turned
// by a quarter: it takes one frame, asks RecognizePlaceInMaps from which of the saved positions the maps look like that
// frame, starts from the best candidate's guess (SetWorldTransformFromGuess) and localizes the following frames.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_relocalization.cpp -Llidarslam_amd -llidarslam_amd
//       -Wl,-rpath,$PWD/lidarslam_amd -o slam_relocalization          (one command line)
//   ./slam_relocalization <prefix> [model=16] [mapped=30] [query=17] [localized=6]
// prints "# candidate <viewpoint> <distance> <shift> <yaw>" of every candidate, "# guess x y z" of the one taken, "# mapped x y z"
// of the mapping pose of the query's place, then "frame x y z" of every localized pose
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "LidarSlam/Slam.h"

// frame f of the drive (seed 1000) or of a second scan of the same places (seed 1001), the base turned by +90 degrees
static LidarSlam::Slam::PointCloud::Ptr Frame(int model, int seed, int f, bool quarterTurn, int seq)
{
  LidarSlam::Slam::PointCloud::Ptr pc(new LidarSlam::Slam::PointCloud);
  pc->points.resize(1 << 19);
  std::uint64_t stamp = 0;
  lsa_point_t* pts = reinterpret_cast<lsa_point_t*>(pc->points.data());
  const int n = lsa_synth_frame(model, seed, f, pts, (int)pc->points.size(), &stamp);
  pc->points.resize(n > 0 ? n : 0);
  if (quarterTurn)
    for (int i = 0; i < n; ++i)
    {
      const float x = pts[i].x;
      pts[i].x = pts[i].y;
      pts[i].y = -x;
    }
  pc->header.stamp = stamp;
  pc->header.seq = seq;
  return pc;
}

int main(int argc, char** argv)
{
  if (argc < 2)
  {
    std::fprintf(stderr, "usage: %s <prefix> [model] [mapped] [query] [localized]\n", argv[0]);
    return 2;
  }
  const std::string prefix = argv[1];
  const int model = argc > 2 ? std::atoi(argv[2]) : 16;
  const int mapped = argc > 3 ? std::atoi(argv[3]) : 30;
  const int query = argc > 4 ? std::atoi(argv[4]) : 17;
  const int localized = argc > 5 ? std::atoi(argv[5]) : 6;
  try
  {
    {
      LidarSlam::Slam mapper;
      mapper.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
      mapper.SetLoggingTimeout(-1.);  // GetTrajectory() keeps every pose
      for (int f = 0; f < mapped; ++f) mapper.AddFrame(Frame(model, 1000, f, false, f));
      mapper.SaveMapsToPCD(prefix, LidarSlam::PCDFormat::BINARY, false);
      if (!mapper.GetLastError().empty())
      {
        std::fprintf(stderr, "%s\n", mapper.GetLastError().c_str());
        return 3;
      }
      std::ofstream positions(prefix + "positions.txt");
      positions.precision(17);
      for (const LidarSlam::Transform& t : mapper.GetTrajectory()) positions << t.x() << " " << t.y() << " " << t.z() << "\n";
    }
    std::vector<std::array<double, 3>> viewpoints;
    {
      std::ifstream positions(prefix + "positions.txt");
      std::array<double, 3> v;
      while (positions >> v[0] >> v[1] >> v[2]) viewpoints.push_back(v);
    }
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetMapUpdate(LidarSlam::MappingMode::NONE);  // the loaded points are fixed, nothing is added
    slam.LoadMapsFromPCD(prefix);
    if (!slam.GetLastError().empty())
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    // switched on at the place of mapping frame `query`, the base turned: the first frame gives the keypoints to recognise by
    // (its own pose, registered from the origin, means nothing)
    slam.AddFrame(Frame(model, 1001, query, true, 0));
    LidarSlam::Slam::MapPlaceSummary summary;
    const std::vector<LidarSlam::Slam::MapPlaceCandidate> found = slam.RecognizePlaceInMaps(viewpoints, LidarSlam::Slam::DefaultMapPlaceSearchParameters(), 3, &summary);
    if (found.empty())
    {
      std::fprintf(stderr, "no place recognised: %s\n", slam.GetLastError().c_str());
      return 3;
    }
    std::printf("# described %d %d\n", summary.viewpoints, summary.described);
    for (const LidarSlam::Slam::MapPlaceCandidate& c : found) std::printf("# candidate %d %.9g %d %.17g\n", c.viewpoint, c.distance, c.shift, c.yaw);
    std::array<double, 16> guess;
    for (int i = 0; i < 16; ++i) guess[i] = found[0].guess[i];
    std::printf("# guess %.12f %.12f %.12f\n", guess[3], guess[7], guess[11]);
    if (query < (int)viewpoints.size()) std::printf("# mapped %.12f %.12f %.12f\n", viewpoints[query][0], viewpoints[query][1], viewpoints[query][2]);
    slam.SetWorldTransformFromGuess(LidarSlam::Transform(guess));
    for (int f = query + 1; f <= query + localized; ++f)
    {
      slam.AddFrame(Frame(model, 1001, f, true, f - query));
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
