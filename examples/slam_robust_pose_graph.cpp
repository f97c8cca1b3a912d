// Pose-graph optimization of a logged trajectory with a FALSE loop edge among the constraints, under a robust loss; written
// against the reference's C++ API and linked with liblidarslam_amd.so.  The drive is slam_pose_graph.cpp's: N frames forward
// with the keypoint log on (SetLoggingTimeout(-1)), then the same clouds in reverse order.  RecognizePlace and
// RegisterLoggedFrames give the true loop-closure edge; a second edge claims the same revisit 30 m away from frame 3 -- what a
// false place match followed by a confident registration looks like.  OptimizeLoggedTrajectory solves the graph twice: without
// a loss (the false edge bends the whole trajectory; nothing is applied) and under Tukey's loss at 3 sigmas (the false edge's
// verdict weight is 0, the true one's stays near 1; the maps are rebuilt under that result); two more frames are then added.
// A registration is trusted to 0.1 m / 0.02 rad here, not to the millimetres its own covariance claims: under those the drift
// of the odometry alone is tens of sigmas and a loss would discount the true loop as well.
//   g++ -std=c++17 -Iinclude -Ilidarslam_amd/include examples/slam_robust_pose_graph.cpp
//       -Llidarslam_amd -llidarslam_amd -Wl,-rpath,$PWD/lidarslam_amd -o slam_robust_pose_graph      (one command line)
//   ./slam_robust_pose_graph [model=16] [forward=12]
// prints "# edge <revisited> <query>" for both edges, and per solve (loss 0, then loss 3) "# solve <loss> <termination> <LM
// iterations> <PCG iterations>", "# cost <initial> <final>", "# verdict <loss> <edge> <chi2> <weight>" per loop edge, "# last x y z"
// (the optimized last pose's position); then "# frame x y z" for each of the two frames added afterwards
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
    search.min_travelled = 2.;
    search.max_distance = 0.;
    search.exclusion_half_window = 2;
    const std::vector<LidarSlam::Slam::PlaceCandidate> found = slam.RecognizePlace(query, search, 3);
    if (found.empty())
    {
      std::fprintf(stderr, "no candidate: %s\n", slam.GetLastError().c_str());
      return 2;
    }
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
    if (reg.status != 0)
    {
      std::fprintf(stderr, "not registered (%d): %s\n", reg.status, slam.GetLastError().c_str());
      return 3;
    }

    std::vector<LidarSlam::Slam::PoseGraphEdge> edges(2);
    if (!LidarSlam::Slam::LoopClosureEdge(found[0].frame, query, reg, edges[0]))
    {
      std::fprintf(stderr, "the registration's covariance is not positive definite\n");
      return 4;
    }
    // the false edge: frame 3 -> query as the logged poses have it, moved by (18, -24, 0) m
    edges[1] = edges[0];
    edges[1].from = 3;
    const std::array<double, 16>&A = poses[3].matrix, &B = poses[query].matrix;
    for (int i = 0; i < 3; ++i)
    {
      for (int j = 0; j < 3; ++j) edges[1].relative[4 * i + j] = A[i] * B[j] + A[4 + i] * B[4 + j] + A[8 + i] * B[8 + j];
      edges[1].relative[4 * i + 3] = A[i] * (B[3] - A[3]) + A[4 + i] * (B[7] - A[7]) + A[8 + i] * (B[11] - A[11]);
    }
    edges[1].relative[3] += 18.;
    edges[1].relative[7] -= 24.;
    for (LidarSlam::Slam::PoseGraphEdge& edge : edges)
    {
      for (double& v : edge.information) v = 0.;
      for (int k = 0; k < 6; ++k) edge.information[7 * k] = k < 3 ? 1. / (0.1 * 0.1) : 1. / (0.02 * 0.02);
      std::printf("# edge %d %d\n", edge.from, edge.to);
    }
    for (int loss : {LSA_PGO_LOSS_NONE, LSA_PGO_LOSS_TUKEY})
    {
      LidarSlam::Slam::PoseGraphParameters pgo = LidarSlam::Slam::DefaultPoseGraphParameters();
      pgo.apply = loss == LSA_PGO_LOSS_TUKEY;  // the maps are rebuilt under the robust result alone
      LidarSlam::Slam::RobustParameters robust = LidarSlam::Slam::DefaultRobustParameters();
      robust.edge_loss = loss;
      robust.edge_scale = 3.;
      LidarSlam::Slam::PoseGraphSummary summary;
      std::vector<LidarSlam::Slam::ConstraintVerdict> verdicts;
      const std::vector<LidarSlam::Transform> optimized = slam.OptimizeLoggedTrajectory(edges, pgo, robust, &summary, &verdicts);
      if (optimized.empty())
      {
        std::fprintf(stderr, "%s\n", slam.GetLastError().c_str());
        return 5;
      }
      std::printf("# solve %d %d %d %d\n", loss, summary.termination, summary.iterations, summary.pcg_iterations);
      std::printf("# cost %.9g %.9g\n", summary.initial_cost, summary.final_cost);
      for (std::size_t k = 0; k < verdicts.size(); ++k) std::printf("# verdict %d %d %.9g %.9g\n", loss, (int)k, verdicts[k].chi2, verdicts[k].weight);
      std::printf("# last %.12f %.12f %.12f\n", optimized.back().matrix[3], optimized.back().matrix[7], optimized.back().matrix[11]);
    }
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
