// Place recognition on the keypoint log, written against the reference's C++ API and linked with liblidarslam_amd.so.  A Slam
// maps N frames forward with the keypoint log on (SetLoggingTimeout(-1)) and then the same clouds in reverse order: the
// vehicle backs up over its own track.  RecognizePlace names the logged frames that LOOK like the last one -- descriptors of
// the logged keypoints, built and compared on the device; no position is consulted -- with the yaw between the two;
// RegisterLoggedFrames registers the last frame against the log around the best of them, from the guess
// pose[candidate] * Rz(yaw), and returns the edge candidate -> last a pose-graph optimizer takes.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_place_recognition.cpp
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_place_recognition      (one command line)
//   ./slam_place_recognition [model=16] [forward=12]
// prints "# query <frame>", one "# candidate <frame> <distance> <shift> <yaw [rad]>" per candidate, best first,
// "# registered <status> <iterations>", "# relative x y z" (the edge's translation) and "# errors <position [m]> <orientation [deg]>"
#include <array>
#include <cmath>
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

    const int query = seq - 1;
    LidarSlam::Slam::PlaceSearchParameters search = LidarSlam::Slam::DefaultPlaceSearchParameters();
    search.min_travelled = 2.;         // [m] back along the trajectory: the frames just before the query are no revisit
    search.max_distance = 0.;          // no position gate: the descriptors decide
    search.exclusion_half_window = 2;  // one candidate per place
    const std::vector<LidarSlam::Slam::PlaceCandidate> found = slam.RecognizePlace(query, search, 3);
    std::printf("# query %d\n", query);
    for (const LidarSlam::Slam::PlaceCandidate& c : found) std::printf("# candidate %d %.9g %d %.17g\n", c.frame, c.distance, c.shift, c.yaw);
    if (found.empty())
    {
      std::fprintf(stderr, "no candidate: %s\n", slam.GetLastError().c_str());
      return 2;
    }

    // the guess: the candidate's logged pose turned by the yaw the descriptors found
    const std::vector<LidarSlam::Transform> poses = slam.GetTrajectory();
    const std::array<double, 16>& P = poses[found[0].frame].matrix;
    const double c = std::cos(found[0].yaw), s = std::sin(found[0].yaw);
    LidarSlam::Transform guess = poses[found[0].frame];
    for (int i = 0; i < 3; ++i)
    {
      guess.matrix[4 * i] = P[4 * i] * c + P[4 * i + 1] * s;
      guess.matrix[4 * i + 1] = -P[4 * i] * s + P[4 * i + 1] * c;
    }
    LidarSlam::Slam::LoopClosureParameters params = LidarSlam::Slam::DefaultLoopClosureParameters();
    params.revisited_half_window = 2;
    const LidarSlam::Slam::LoopClosureRegistration reg = slam.RegisterLoggedFrames(query, found[0].frame, params, &guess);
    if (reg.status < 0)
    {
      std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
      return 3;
    }
    std::printf("# registered %d %d\n", reg.status, reg.iterations);
    std::printf("# relative %.12f %.12f %.12f\n", reg.relative[3], reg.relative[7], reg.relative[11]);
    std::printf("# errors %.9f %.9f\n", reg.position_error, reg.orientation_error);
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
