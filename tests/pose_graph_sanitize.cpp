// Driver of tests/test_host_pose_graph.py: the host statement of the pose-graph solve (lidarslam_amd/csrc/host/lsa_pose_graph.cpp
// over lsa_pose_graph.h) compiled with its own main under -fsanitize=address,undefined.  Runs laps of 2, 3, 16, 64 and 200
// poses with one to three loop edges, the seams, the refusals and the degenerate inputs, checks the answers that can be
// stated in a line, and prints "ok".
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

struct Lap
{
  std::vector<double> poses;  // exactly 16 n, so that a read or write past the end is the sanitizer's to find
  std::vector<unsigned char> fixed;
  std::vector<lsa_pgo_edge_t> edges;
};

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
static pg::Pose Between(const pg::Pose& a, const pg::Pose& b)
{
  pg::Pose z;
  double dt[3];
  for (int k = 0; k < 3; ++k) dt[k] = b.t[k] - a.t[k];
  pg::tmulv3(a.R, dt, z.t);
  pg::tmul3(a.R, b.R, z.R);
  return z;
}
static pg::Pose Compose(const pg::Pose& a, const pg::Pose& z)
{
  const double d[6] = {z.t[0], z.t[1], z.t[2], 0, 0, 0};
  pg::Pose r = pg::retract(a, d);  // t = a.t + a.R z.t
  pg::mul3(a.R, z.R, r.R);
  return r;
}

static Lap MakeLap(int n, const std::vector<std::pair<int, int>>& loops, unsigned seed)
{
  std::mt19937 gen(seed);
  std::normal_distribution<double> normal(0., 1.);
  const bool small = n < 16;
  const double scale = small ? 5. : 1.;
  std::vector<pg::Pose> truth;
  for (int i = 0; i < n; ++i) truth.push_back(CirclePose(2 * 3.141592653589793 * i / (n < 16 ? 16 : n)));
  Lap lap;
  lap.poses.resize(static_cast<size_t>(n) * 16);
  lap.fixed.assign(static_cast<size_t>(n), 0);
  lap.fixed[0] = 1;
  pg::Pose at = truth[0];
  pg::store(at, &lap.poses[0]);
  auto info = [](lsa_pgo_edge_t& e, double f) {
    std::memset(e.information, 0, sizeof(e.information));
    for (int k = 0; k < 6; ++k) e.information[k * 7] = (k < 3 ? 1e4 : 2.5e5) * f;
  };
  for (int i = 1; i < n; ++i)
  {
    double noise[6];
    for (int k = 0; k < 6; ++k) noise[k] = (k < 3 ? 0.01 : 0.002) * scale * normal(gen);
    const pg::Pose z = pg::retract(Between(truth[i - 1], truth[i]), noise);
    lsa_pgo_edge_t e;
    e.from = i - 1;
    e.to = i;
    pg::store(z, e.relative);
    info(e, small ? 1. / 25. : 1.);
    lap.edges.push_back(e);
    at = Compose(at, z);
    pg::store(at, &lap.poses[16 * static_cast<size_t>(i)]);
  }
  for (const auto& l : loops)
  {
    lsa_pgo_edge_t e;
    e.from = l.first;
    e.to = l.second;
    pg::store(Between(truth[l.first], truth[l.second]), e.relative);
    info(e, small ? 100. : 1.);
    lap.edges.push_back(e);
  }
  return lap;
}

static bool AllFinite(const std::vector<double>& v)
{
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

static void Solve(int n, const std::vector<std::pair<int, int>>& loops)
{
  const Lap lap = MakeLap(n, loops, 1000u + n);
  const int m = static_cast<int>(lap.edges.size());
  std::vector<double> out(static_cast<size_t>(n) * 16, -7.);
  lsa_pgo_result_t r;
  std::memset(&r, 0, sizeof(r));
  CHECK(lsa_pgo_solve_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, nullptr, out.data(), &r) == LSA_OK);
  CHECK(AllFinite(out));
  CHECK(r.termination == LSA_PGO_STEP || r.termination == LSA_PGO_COST || r.termination == LSA_PGO_GRADIENT);
  CHECK(r.final_cost < 0.1 * r.initial_cost);
  CHECK(std::memcmp(out.data(), lap.poses.data(), 16 * sizeof(double)) == 0);
  // in place
  std::vector<double> inplace = lap.poses;
  CHECK(lsa_pgo_solve_host(inplace.data(), n, lap.fixed.data(), lap.edges.data(), m, nullptr, inplace.data(), &r) == LSA_OK);
  CHECK(std::memcmp(inplace.data(), out.data(), out.size() * sizeof(double)) == 0);
  // the preconditioner reduced to its diagonal blocks, and one PCG iteration a step
  lsa_pgo_params_t p;
  lsa_pgo_params_init(&p);
  p.preconditioner = 1;
  p.pcg_max_iter = 5000;
  CHECK(lsa_pgo_solve_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, &p, inplace.data(), &r) == LSA_OK);
  CHECK(r.final_cost < 0.1 * r.initial_cost);
  lsa_pgo_params_init(&p);
  p.pcg_max_iter = 1;
  p.max_iterations = 6;
  CHECK(lsa_pgo_solve_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, &p, inplace.data(), &r) == LSA_OK);
  CHECK(AllFinite(inplace) && r.termination != LSA_PGO_LINEAR_SOLVER_FAILED);
  // the seams, every output exactly as long as the header says
  std::vector<double> e(static_cast<size_t>(m) * 6), blocks(static_cast<size_t>(m) * pg::kEdgeBlock), chi2(static_cast<size_t>(m));
  CHECK(lsa_pgo_linearize_host(lap.poses.data(), n, lap.edges.data(), m, e.data(), blocks.data(), chi2.data()) == LSA_OK);
  std::vector<double> D(static_cast<size_t>(n) * 36), L(D.size()), U(D.size()), g(static_cast<size_t>(n) * 6), x(g.size(), -7.), q(g.size());
  CHECK(lsa_pgo_assemble_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, 1e-3, D.data(), g.data(), L.data(), U.data()) == LSA_OK);
  CHECK(lsa_pgo_tridiagonal_solve_host(n, D.data(), L.data(), U.data(), g.data(), x.data()) == LSA_OK);
  CHECK(AllFinite(x));
  CHECK(lsa_pgo_spmv_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, 1e-3, x.data(), q.data()) == LSA_OK);
  CHECK(lsa_pgo_retract_host(lap.poses.data(), n, x.data(), out.data()) == LSA_OK);
  double e6[6], A[36], B[36];
  CHECK(lsa_pgo_edge_jacobians_host(lap.poses.data(), n, &lap.edges.back(), e6, A, B) == LSA_OK);
  // an indefinite block
  for (int k = 0; k < 36; ++k) D[static_cast<size_t>(n / 2) * 36 + k] = -D[static_cast<size_t>(n / 2) * 36 + k];
  std::fill(x.begin(), x.end(), -7.);
  CHECK(lsa_pgo_tridiagonal_solve_host(n, D.data(), L.data(), U.data(), g.data(), x.data()) == 1);
  for (double v : x) CHECK(v == -7.);
}

static void Refusals()
{
  Lap lap = MakeLap(16, {{2, 15}}, 7);
  const int n = 16, m = static_cast<int>(lap.edges.size());
  std::vector<double> out(static_cast<size_t>(n) * 16, -7.);
  lsa_pgo_result_t r;
  std::memset(&r, 0, sizeof(r));
  r.iterations = -7;
  auto refused = [&](const Lap& g, int nn, int mm) {
    CHECK(lsa_pgo_solve_host(g.poses.data(), nn, g.fixed.data(), g.edges.data(), mm, nullptr, out.data(), &r) == LSA_E_ARG);
    for (double v : out) CHECK(v == -7.);
    CHECK(r.iterations == -7);
  };
  Lap g = lap;
  g.fixed[0] = 0;
  refused(g, n, m);  // no fixed pose
  g = lap;
  g.edges.erase(g.edges.begin() + 6, g.edges.begin() + 8);  // pose 7 without an edge
  refused(g, n, m - 2);
  g = lap;
  g.edges[3].to = n;
  refused(g, n, m);
  g.edges[3].to = -1;
  refused(g, n, m);
  g.edges[3].to = g.edges[3].from;
  refused(g, n, m);
  g = lap;
  g.poses[16 * 5 + 7] = std::numeric_limits<double>::quiet_NaN();
  refused(g, n, m);
  g = lap;
  g.edges[2].information[8] = std::numeric_limits<double>::infinity();
  refused(g, n, m);
  g = lap;
  g.edges[2].relative[3] = std::numeric_limits<double>::quiet_NaN();
  refused(g, n, m);
  refused(lap, 0, 0);
  CHECK(lsa_pgo_solve_host(nullptr, n, lap.fixed.data(), lap.edges.data(), m, nullptr, out.data(), &r) == LSA_E_ARG);
  lsa_pgo_params_t p;
  lsa_pgo_params_init(&p);
  p.pcg_tolerance = 0.;
  CHECK(lsa_pgo_solve_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, &p, out.data(), &r) == LSA_E_ARG);
  // every pose fixed, no edge: nothing to do, and said so
  std::vector<unsigned char> all(static_cast<size_t>(n), 1);
  CHECK(lsa_pgo_solve_host(lap.poses.data(), n, all.data(), nullptr, 0, nullptr, out.data(), &r) == LSA_OK);
  CHECK(r.termination == LSA_PGO_GRADIENT && std::memcmp(out.data(), lap.poses.data(), out.size() * sizeof(double)) == 0);
  // a loop edge a kilometre off: ends by a rule
  g = lap;
  g.edges.back().relative[3] += 1000.;
  lsa_pgo_params_init(&p);
  p.max_iterations = 30;
  CHECK(lsa_pgo_solve_host(g.poses.data(), n, g.fixed.data(), g.edges.data(), m, &p, out.data(), &r) == LSA_OK);
  CHECK(AllFinite(out) && r.iterations <= 30 && std::isfinite(r.final_cost));
  // covariances
  double cov[36], info[36];
  std::memset(cov, 0, sizeof(cov));
  for (int k = 0; k < 6; ++k) cov[k * 7] = 1e-4 * (k + 1);
  cov[1] = cov[6] = 2e-5;
  CHECK(lsa_pgo_information_from_covariance(cov, info) == LSA_OK);
  cov[14] = -1.;
  CHECK(lsa_pgo_information_from_covariance(cov, info) == LSA_E_ARG);
  std::memset(cov, 0, sizeof(cov));
  CHECK(lsa_pgo_information_from_covariance(cov, info) == LSA_E_ARG);
}

int main()
{
  Solve(2, {{0, 1}});
  Solve(3, {{0, 2}});
  Solve(16, {{2, 15}});
  Solve(64, {{3, 63}});
  Solve(200, {{1, 199}, {10, 150}, {50, 120}});
  Refusals();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
