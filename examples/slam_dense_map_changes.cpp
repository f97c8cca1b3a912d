// What is new in the frame in hand: a short synthetic drive is mapped with the dense point-cloud map, then a box of points that
// no earlier frame holds -- the parked car that arrived -- is added to the next frame, and CompareFrameToDenseMap labels every
// point of that frame against the map as it stood before it: the box's points come out UNMAPPED.  Then the map is rendered as
// a 16 x 360 scan from the current pose.  Written against the reference's C++ API and linked with liblidarslam_amd.so.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_dense_map_changes.cpp \
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_dense_map_changes
//   ./slam_dense_map_changes [model=16] [frames=8] [leaf=0.2] [box points=40]
// prints "# labels <not judged> <consistent> <unmapped> <through map>", "# box <points> <unmapped among them>" and
// "# scan <rays> <hits>"
#include <cstdio>
#include <cstdlib>
#include <string>
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
  const int frames = argc > 2 ? std::atoi(argv[2]) : 8;
  const double leaf = argc > 3 ? std::atof(argv[3]) : 0.2;
  const int box = argc > 4 ? std::atoi(argv[4]) : 40;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    slam.SetDenseMapLeafSize(leaf);
    slam.SetDenseMap(1);  // every registered frame
    for (int f = 0; f < frames; ++f) slam.AddFrame(Frame(model, f));
    // the next frame, and in it a box of a metre 6 m ahead of the sensor that was in no frame before
    LidarSlam::Slam::PointCloud::Ptr pc = Frame(model, frames);
    const std::size_t own = pc->points.size();
    for (int i = 0; i < box; ++i)
    {
      LidarSlam::Slam::Point p = pc->points[own / 2];
      p.x = 5.5f + static_cast<float>(i % 5) * 0.25f;
      p.y = -0.5f + static_cast<float>((i / 5) % 4) * 0.33f;
      p.z = -0.5f + static_cast<float>(i / 20) * 0.9f;
      p.laser_id = static_cast<std::uint16_t>(i % 16);
      pc->points.push_back(p);
    }
    slam.AddFrame(pc);
    long long counts[4] = {0, 0, 0, 0};
    const std::vector<std::uint8_t> labels = slam.CompareFrameToDenseMap(counts);
    if (labels.size() != pc->points.size())
    {
      std::fprintf(stderr, "CompareFrameToDenseMap: %zu labels for %zu points: %s\n", labels.size(), pc->points.size(), slam.GetLastError().c_str());
      return 3;
    }
    long long unmapped = 0;
    for (std::size_t i = own; i < labels.size(); ++i) unmapped += labels[i] == LidarSlam::Slam::DENSE_UNMAPPED;
    std::printf("# labels %lld %lld %lld %lld\n", counts[0], counts[1], counts[2], counts[3]);
    std::printf("# box %d %lld\n", box, unmapped);
    // the map as a VLP-16 would see it from here
    std::vector<double> elevations;
    for (int r = 0; r < 16; ++r) elevations.push_back((-15. + 2. * r) * (3.14159265358979323846 / 180.));
    const std::vector<LidarSlam::Slam::DenseHit> scan = slam.RenderDenseMapScan(elevations, 360);
    if (scan.size() != 16u * 360u)
    {
      std::fprintf(stderr, "RenderDenseMapScan: %s\n", slam.GetLastError().c_str());
      return 3;
    }
    long long hit = 0;
    for (const LidarSlam::Slam::DenseHit& h : scan) hit += h.status == 1;
    std::printf("# scan %zu %lld\n", scan.size(), hit);
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
