// Driver of tests/test_pose_graph_priors_host.py: the host statement of the pose-graph solve with position priors
// (lidarslam_amd/csrc/host/lsa_pose_graph.cpp over lsa_pose_graph.h), the GPS matcher and the track alignment
// (host/lsa_gps.cpp) compiled with their own main under -fsanitize=address,undefined.  Runs laps of 3, 16, 64 and 200 free poses
// with a prior every few poses, the seams, the refusals, the matcher and the alignment on the shapes of the tests, checks the
// answers that can be stated in a line, and prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "lsa_pose_graph.h"

namespace pg = lsa::pg;

static int failures = 0;
#define CHECK(cond)                                                 \
  do                                                                \
  {                                                                 \
    if (!(cond))                                                    \
    {                                                               \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static pg::Pose CirclePose(double a)
{
  const double yaw[3] = {0., 0., a + 1.5707963267948966}, tilt[3] = {0.03 * std::sin(3 * a), 0.02 * std::cos(2 * a), 0.};
  double Rz[9], Rt[9];
  pg::so3_exp(yaw, Rz);
  pg::so3_exp(tilt, Rt);
  pg::Pose p;
  pg::mul3(Rz, Rt, p.R);
  p.t[0] = 20. * std::cos(a); p.t[1] = 20. * std::sin(a); p.t[2] = 0.5 * std::sin(a);
  return p;
}

struct Case
{
  std::vector<double> poses;  // exactly 16 n, so that a read or write past the end is the sanitizer's to find
  std::vector<unsigned char> fixed;
  std::vector<lsa_pgo_edge_t> edges;
  std::vector<lsa_pgo_prior_t> priors;
  double offset[16];
};

static bool AllFinite(const std::vector<double>& v)
{
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

// a lap of n free poses in the frame of the fixes, noisy odometry, a prior every `every` poses
static Case MakeCase(int n, int every, unsigned seed)
{
  std::mt19937 gen(seed);
  std::normal_distribution<double> normal(0., 1.);
  Case c;
  pg::Pose O, Wt;
  const double lever[3] = {0.1, -0.2, 0.3}, yaw[3] = {0.02, -0.03, 0.8};
  pg::so3_exp(lever, O.R);
  O.t[0] = 0.4; O.t[1] = -0.3; O.t[2] = 1.2;
  pg::store(O, c.offset);
  pg::so3_exp(yaw, Wt.R);
  Wt.t[0] = 100.; Wt.t[1] = -50.; Wt.t[2] = 10.;
  std::vector<pg::Pose> truth;
  for (int i = 0; i < n; ++i) truth.push_back(pg::compose(Wt, CirclePose(2 * 3.141592653589793 * i / (n < 16 ? 16 : n))));
  c.poses.resize(static_cast<size_t>(n) * 16);
  c.fixed.assign(static_cast<size_t>(n), 0);
  pg::Pose at = truth[0];
  pg::store(at, &c.poses[0]);
  for (int i = 1; i < n; ++i)
  {
    double noise[6];
    for (int k = 0; k < 6; ++k) noise[k] = (k < 3 ? 0.01 : 0.002) * normal(gen);
    const pg::Pose z = pg::retract(pg::inverse_compose(truth[i - 1], truth[i]), noise);
    lsa_pgo_edge_t e;
    e.from = i - 1;
    e.to = i;
    pg::store(z, e.relative);
    std::memset(e.information, 0, sizeof(e.information));
    for (int k = 0; k < 6; ++k) e.information[k * 7] = k < 3 ? 1e4 : 2.5e5;
    c.edges.push_back(e);
    at = pg::compose(at, z);
    pg::store(at, &c.poses[16 * static_cast<size_t>(i)]);
  }
  for (int i = 0; i < n; i += every)
  {
    lsa_pgo_prior_t p;
    std::memset(&p, 0, sizeof(p));
    p.pose = i;
    const pg::Pose antenna = pg::compose(truth[i], O);
    for (int k = 0; k < 3; ++k) p.position[k] = antenna.t[k] + 0.03 * normal(gen);
    for (int k = 0; k < 3; ++k) p.information[k * 4] = 1. / (0.03 * 0.03);
    c.priors.push_back(p);
  }
  return c;
}

static void Solve(int n, int every)
{
  const Case c = MakeCase(n, every, 2000u + n);
  const int m = static_cast<int>(c.edges.size()), k = static_cast<int>(c.priors.size());
  std::vector<double> out(static_cast<size_t>(n) * 16, -7.);
  lsa_pgo_result_t r;
  std::memset(&r, 0, sizeof(r));
  CHECK(lsa_pgo_solve_priors_host(c.poses.data(), n, c.fixed.data(), c.edges.data(), m, c.priors.data(), k, c.offset, nullptr, out.data(), &r) == LSA_OK);
  CHECK(AllFinite(out));
  CHECK(r.termination == LSA_PGO_STEP || r.termination == LSA_PGO_COST || r.termination == LSA_PGO_GRADIENT);
  CHECK(r.final_cost < r.initial_cost);
  // in place
  std::vector<double> inplace = c.poses;
  CHECK(lsa_pgo_solve_priors_host(inplace.data(), n, c.fixed.data(), c.edges.data(), m, c.priors.data(), k, c.offset, nullptr, inplace.data(), &r) == LSA_OK);
  CHECK(std::memcmp(inplace.data(), out.data(), out.size() * sizeof(double)) == 0);
  // no prior, pose 0 fixed: the bits of the call without priors
  std::vector<unsigned char> first(static_cast<size_t>(n), 0);
  first[0] = 1;
  std::vector<double> a(out.size()), b(out.size());
  lsa_pgo_result_t ra, rb;
  CHECK(lsa_pgo_solve_host(c.poses.data(), n, first.data(), c.edges.data(), m, nullptr, a.data(), &ra) == LSA_OK);
  CHECK(lsa_pgo_solve_priors_host(c.poses.data(), n, first.data(), c.edges.data(), m, nullptr, 0, nullptr, nullptr, b.data(), &rb) == LSA_OK);
  CHECK(std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0 && ra.iterations == rb.iterations);
  // the seams, every output exactly as long as the header says
  std::vector<double> e(static_cast<size_t>(k) * 3), blocks(static_cast<size_t>(k) * pg::kPriorBlock), chi2(static_cast<size_t>(k));
  CHECK(lsa_pgo_linearize_priors_host(c.poses.data(), n, c.priors.data(), k, c.offset, e.data(), blocks.data(), chi2.data()) == LSA_OK);
  std::vector<double> D(static_cast<size_t>(n) * 36), L(D.size()), U(D.size()), g(static_cast<size_t>(n) * 6), x(g.size(), -7.), q(g.size());
  CHECK(lsa_pgo_assemble_priors_host(c.poses.data(), n, c.fixed.data(), c.edges.data(), m, c.priors.data(), k, c.offset, 1e-3, D.data(), g.data(), L.data(), U.data()) == LSA_OK);
  CHECK(lsa_pgo_tridiagonal_solve_host(n, D.data(), L.data(), U.data(), g.data(), x.data()) == LSA_OK);
  CHECK(AllFinite(x));
  CHECK(lsa_pgo_spmv_priors_host(c.poses.data(), n, c.fixed.data(), c.edges.data(), m, c.priors.data(), k, c.offset, 1e-3, x.data(), q.data()) == LSA_OK);
  double e3[3], A[18];
  CHECK(lsa_pgo_prior_jacobian_host(c.poses.data(), n, &c.priors.back(), c.offset, e3, A) == LSA_OK);
  double W[16];
  pg::store(CirclePose(0.3), W);
  CHECK(lsa_pgo_premultiply_host(c.poses.data(), n, W, out.data()) == LSA_OK);
  CHECK(lsa_pgo_reanchor_host(out.data(), n, out.data()) == LSA_OK);  // in place
  CHECK(std::fabs(out[0] - 1.) < 1e-15 && std::fabs(out[3]) < 1e-13);
}

static void Refusals()
{
  Case c = MakeCase(16, 3, 7);
  const int n = 16, m = static_cast<int>(c.edges.size()), k = static_cast<int>(c.priors.size());
  std::vector<double> out(static_cast<size_t>(n) * 16, -7.);
  lsa_pgo_result_t r;
  std::memset(&r, 0, sizeof(r));
  r.iterations = -7;
  auto refused = [&](const Case& g, int kk, const double* offset) {
    CHECK(lsa_pgo_solve_priors_host(g.poses.data(), n, g.fixed.data(), g.edges.data(), m, g.priors.data(), kk, offset, nullptr, out.data(), &r) == LSA_E_ARG);
    for (double v : out) CHECK(v == -7.);
    CHECK(r.iterations == -7);
  };
  refused(c, 0, c.offset);   // no fixed pose and no prior
  refused(c, -1, c.offset);
  refused(c, k, nullptr);
  Case g = c;
  g.priors[1].pose = n;
  refused(g, k, c.offset);
  g.priors[1].pose = -1;
  refused(g, k, c.offset);
  g = c;
  g.priors[2].position[1] = std::numeric_limits<double>::quiet_NaN();
  refused(g, k, c.offset);
  g = c;
  g.priors[0].information[4] = std::numeric_limits<double>::infinity();
  refused(g, k, c.offset);
  g = c;
  g.offset[7] = std::numeric_limits<double>::quiet_NaN();
  refused(g, k, g.offset);
  // a prior on a fixed pose, and an indefinite information: legal, ends by a rule
  g = c;
  g.fixed[0] = 1;
  g.priors[3].information[0] = -1.;
  lsa_pgo_params_t p;
  lsa_pgo_params_init(&p);
  p.max_iterations = 20;
  CHECK(lsa_pgo_solve_priors_host(g.poses.data(), n, g.fixed.data(), g.edges.data(), m, g.priors.data(), k, g.offset, &p, out.data(), &r) == LSA_OK);
  CHECK(AllFinite(out) && r.iterations <= 20 && std::memcmp(out.data(), g.poses.data(), 16 * sizeof(double)) == 0);
  // covariances
  double cov[9] = {4e-4, 1e-5, 0., 1e-5, 9e-4, 0., 0., 0., 2.5e-3}, info[9];
  CHECK(lsa_pgo_information_from_covariance3(cov, info) == LSA_OK && std::fabs(info[8] - 400.) < 1e-9);
  cov[8] = -1.;
  CHECK(lsa_pgo_information_from_covariance3(cov, info) == LSA_E_ARG);
  std::memset(cov, 0, sizeof(cov));
  CHECK(lsa_pgo_information_from_covariance3(cov, info) == LSA_E_ARG);
}

static void Matcher()
{
  std::vector<double> slam, gps;
  for (int i = 0; i < 40; ++i) slam.push_back(100. + 0.1 * i);
  for (int i = 0; i < 300; ++i) gps.push_back(99.85 + 0.014 * i);
  std::vector<int32_t> match(gps.size(), -2);  // exactly G
  CHECK(lsa_gps_match_trajectory(slam.data(), 40, gps.data(), 300, 0., 0.1, match.data()) == LSA_OK);
  int accepted = 0, last = -1;
  for (int32_t v : match)
  {
    CHECK(v >= -1 && v < 40);
    if (v >= 0) { CHECK(v > last); last = v; ++accepted; }
  }
  CHECK(accepted == 40);
  const double grid[4] = {10., 10.5, 11., 11.5}, fixes[3] = {9., 10.25, 12.};
  int32_t three[3];
  CHECK(lsa_gps_match_trajectory(grid, 4, fixes, 3, 0., 0.25, three) == LSA_OK && three[0] == -1 && three[1] == 0 && three[2] == -1);
  CHECK(lsa_gps_match_trajectory(grid, 4, fixes, 3, 0., 0.5, three) == LSA_OK && three[0] == -1 && three[1] == 0 && three[2] == 3);
  CHECK(lsa_gps_match_trajectory(grid, 0, fixes, 3, 0., 0.5, three) == LSA_OK && three[0] == -1 && three[2] == -1);
  CHECK(lsa_gps_match_trajectory(grid, 4, fixes, 0, 0., 0.5, nullptr) == LSA_OK);
  const double backwards[2] = {2., 1.};
  CHECK(lsa_gps_match_trajectory(backwards, 2, fixes, 3, 0., 0.5, three) == LSA_E_ARG);
  CHECK(lsa_gps_match_trajectory(grid, 4, fixes, 3, 0., -1., three) == LSA_E_ARG);
}

static void Alignment()
{
  pg::Pose Wt;
  const double yaw[3] = {0.02, -0.03, 0.8};
  pg::so3_exp(yaw, Wt.R);
  Wt.t[0] = 100.; Wt.t[1] = -50.; Wt.t[2] = 10.;
  for (int kind = 0; kind < 3; ++kind)  // a helix, a planar circle, a line
    for (int pairs : {1, 2, 3, 60})
    {
      std::vector<double> a(static_cast<size_t>(pairs) * 3), b(a.size());  // exactly 3 pairs
      for (int i = 0; i < pairs; ++i)
      {
        const double s = 0.2 * i;
        double* p = &a[3 * static_cast<size_t>(i)];
        if (kind == 2) { p[0] = 1. + 0.6 * s; p[1] = 2.; p[2] = -0.5 + 0.8 * s; }
        else { p[0] = 15. * std::cos(s); p[1] = 15. * std::sin(s); p[2] = kind == 0 ? 0.8 * s : 0.; }
        pg::mulv3(Wt.R, p, &b[3 * static_cast<size_t>(i)]);
        for (int k = 0; k < 3; ++k) b[3 * static_cast<size_t>(i) + k] += Wt.t[k];
      }
      double T[16];
      CHECK(lsa_trajectory_alignment(a.data(), b.data(), pairs, T) == LSA_OK);
      for (double v : T) CHECK(std::isfinite(v));
      if (kind < 2 && pairs == 60)
        for (int r = 0; r < 3; ++r)
        {
          CHECK(std::fabs(T[r * 4 + 3] - Wt.t[r]) < 1e-9);
          for (int cc = 0; cc < 3; ++cc) CHECK(std::fabs(T[r * 4 + cc] - Wt.R[r * 3 + cc]) < 1e-12);
        }
    }
  // opposite chords: half a turn
  const double a[6] = {0., 0., 0., 1., 0., 0.}, b[6] = {5., 5., 5., 4., 5., 5.};
  double T[16];
  CHECK(lsa_trajectory_alignment(a, b, 2, T) == LSA_OK && std::fabs(T[0] + 1.) < 1e-12);
  CHECK(lsa_trajectory_alignment(a, b, 0, T) == LSA_E_ARG);
  CHECK(lsa_trajectory_alignment(nullptr, b, 2, T) == LSA_E_ARG);
}

int main()
{
  Solve(3, 1);
  Solve(16, 3);
  Solve(64, 4);
  Solve(200, 7);
  Refusals();
  Matcher();
  Alignment();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
