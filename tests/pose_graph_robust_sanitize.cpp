// Driver of tests/test_pose_graph_robust_host.py: the host statement of the pose graph under robust losses
// (lidarslam_amd/csrc/host/lsa_pose_graph.cpp over the section ROBUST LOSS of lsa_pose_graph.h) compiled with its own main under
// -fsanitize=address,undefined.  The loss function at the values the Python test takes it through, the weighted
// linearization, a lap of 64 poses with one true and one false loop edge and position priors with one fix 50 m off under every
// loss with its verdicts, and the refusals; checks the answers that can be stated in a line and prints "ok".
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

static void LossValues()
{
  const double scales[3] = {0.5, 1., 3.};
  for (int loss = 0; loss <= 3; ++loss)
    for (double c : scales)
    {
      const double c2 = c * c;
      const double s[9] = {0., 1e-300, 1e-12 * c2, c2 * (1. - std::ldexp(1., -52)), c2, std::nextafter(c2, 1e300), 4. * c2, 1e12 * c2, 5e-324};
      double before = -1.;
      for (int i = 0; i < 9; ++i)
      {
        double rho = -7., w = -7.;
        CHECK(lsa_pgo_robust_rho_host(loss, c, s[i], &rho, &w) == LSA_OK);
        CHECK(std::isfinite(rho) && rho >= 0. && rho <= s[i] * (1. + 1e-15) && w >= 0. && w <= 1.);
        if (i > 0 && i < 8) CHECK(rho >= before * (1. - 1e-15));  // rho does not fall as s grows, to rounding
        before = rho;
        if (loss == LSA_PGO_LOSS_NONE) CHECK(rho == s[i] && w == 1.);
        if (loss == LSA_PGO_LOSS_TUKEY && s[i] > c2) CHECK(rho == c2 / 3. && w == 0.);
        if (loss == LSA_PGO_LOSS_HUBER && !(s[i] > c2)) CHECK(rho == s[i] && w == 1.);
      }
      double rho = 0., w = 0.;
      CHECK(lsa_pgo_robust_rho_host(loss, c, std::numeric_limits<double>::quiet_NaN(), &rho, &w) == LSA_OK && std::isnan(rho));
      CHECK(lsa_pgo_robust_rho_host(loss, c, std::numeric_limits<double>::infinity(), &rho, &w) == LSA_OK);
    }
  double rho = -7., w = -7.;
  CHECK(lsa_pgo_robust_rho_host(4, 1., 1., &rho, &w) == LSA_E_ARG && lsa_pgo_robust_rho_host(-1, 1., 1., &rho, &w) == LSA_E_ARG);
  CHECK(lsa_pgo_robust_rho_host(1, 0., 1., &rho, &w) == LSA_E_ARG && lsa_pgo_robust_rho_host(2, -1., 1., &rho, &w) == LSA_E_ARG);
  CHECK(lsa_pgo_robust_rho_host(3, std::numeric_limits<double>::quiet_NaN(), 1., &rho, &w) == LSA_E_ARG);
  CHECK(lsa_pgo_robust_rho_host(3, std::numeric_limits<double>::infinity(), 1., &rho, &w) == LSA_E_ARG);
  CHECK(lsa_pgo_robust_rho_host(3, 1., 1., nullptr, &w) == LSA_E_ARG && lsa_pgo_robust_rho_host(3, 1., 1., &rho, nullptr) == LSA_E_ARG);
  CHECK(rho == -7. && w == -7.);
  lsa_pgo_robust_t r;
  std::memset(&r, 0xff, sizeof(r));
  lsa_pgo_robust_init(&r);
  lsa_pgo_robust_init(nullptr);
  CHECK(r.edge_loss == LSA_PGO_LOSS_NONE && r.prior_loss == LSA_PGO_LOSS_NONE && r.edge_scale == 1. && r.prior_scale == 1.);
}

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

// every array exactly as long as the header says, so that a read or write past an end is the sanitizer's to find
struct Lap
{
  int n = 0;
  std::vector<double> poses, truth;
  std::vector<unsigned char> fixed, mask;
  std::vector<lsa_pgo_edge_t> edges;
  std::vector<lsa_pgo_prior_t> priors;
  double offset[16];
  int falseEdge = -1, trueEdge = -1, outlier = -1;
};

static Lap MakeLap(int n, bool withPriors)
{
  std::mt19937 gen(900u + n);
  std::normal_distribution<double> normal(0., 1.);
  std::vector<pg::Pose> truth;
  for (int i = 0; i < n; ++i) truth.push_back(CirclePose(2 * 3.141592653589793 * i / n));
  Lap lap;
  lap.n = n;
  lap.poses.resize(static_cast<size_t>(n) * 16);
  lap.fixed.assign(static_cast<size_t>(n), 0);
  lap.fixed[0] = withPriors ? 0 : 1;
  pg::Pose at = truth[0];
  pg::store(at, &lap.poses[0]);
  auto info = [](lsa_pgo_edge_t& e, double sigmaT, double sigmaR) {
    std::memset(e.information, 0, sizeof(e.information));
    for (int k = 0; k < 6; ++k) e.information[k * 7] = 1. / ((k < 3 ? sigmaT : sigmaR) * (k < 3 ? sigmaT : sigmaR));
  };
  for (int i = 1; i < n; ++i)
  {
    double noise[6];
    for (int k = 0; k < 6; ++k) noise[k] = (k < 3 ? 0.002 : 0.0002) * normal(gen);
    const pg::Pose z = pg::retract(Between(truth[i - 1], truth[i]), noise);
    lsa_pgo_edge_t e;
    e.from = i - 1;
    e.to = i;
    pg::store(z, e.relative);
    info(e, 0.002, 0.0002);
    lap.edges.push_back(e);
    const double d[6] = {z.t[0], z.t[1], z.t[2], 0, 0, 0};
    pg::Pose next = pg::retract(at, d);
    pg::mul3(at.R, z.R, next.R);
    at = next;
    pg::store(at, &lap.poses[16 * static_cast<size_t>(i)]);
  }
  const int loops[2][2] = {{3, n - 1}, {n / 6, 2 * n / 3}};
  for (int l = 0; l < 2; ++l)
  {
    lsa_pgo_edge_t e;
    e.from = loops[l][0];
    e.to = loops[l][1];
    pg::Pose z = Between(truth[static_cast<size_t>(e.from)], truth[static_cast<size_t>(e.to)]);
    if (l == 1) { z.t[0] += 30.; z.t[1] -= 40.; }  // the false one: 50 m off
    pg::store(z, e.relative);
    info(e, 0.5, 0.1);
    lap.edges.push_back(e);
  }
  lap.trueEdge = n - 1;
  lap.falseEdge = n;
  lap.mask.assign(lap.edges.size(), 0);
  lap.mask[static_cast<size_t>(n - 1)] = lap.mask[static_cast<size_t>(n)] = 1;
  const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memcpy(lap.offset, eye, sizeof(eye));
  lap.offset[3] = 0.4; lap.offset[7] = -0.3; lap.offset[11] = 1.2;
  if (withPriors)
    for (int i = 0; i < n; i += 4)
    {
      lsa_pgo_prior_t pr;
      std::memset(&pr, 0, sizeof(pr));
      pr.pose = i;
      const double arm[6] = {lap.offset[3], lap.offset[7], lap.offset[11], 0, 0, 0};
      const pg::Pose antenna = pg::retract(truth[static_cast<size_t>(i)], arm);
      for (int k = 0; k < 3; ++k) pr.position[k] = antenna.t[k] + 0.1 * normal(gen);
      for (int k = 0; k < 3; ++k) pr.information[k * 4] = 1. / 0.25;
      if (i == 8) { pr.position[1] += 30.; pr.position[2] += 40.; lap.outlier = static_cast<int>(lap.priors.size()); }
      lap.priors.push_back(pr);
    }
  return lap;
}

static bool AllFinite(const std::vector<double>& v)
{
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

static void SolveUnderEveryLoss(bool withPriors)
{
  const Lap lap = MakeLap(64, withPriors);
  const int n = lap.n, m = static_cast<int>(lap.edges.size()), k = static_cast<int>(lap.priors.size());
  std::vector<double> plain(static_cast<size_t>(n) * 16);
  lsa_pgo_result_t r0;
  CHECK(lsa_pgo_solve_priors_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, k ? lap.priors.data() : nullptr, k, lap.offset, nullptr, plain.data(), &r0) == LSA_OK);
  for (int loss = 0; loss <= 3; ++loss)
  {
    lsa_pgo_robust_t rb;
    lsa_pgo_robust_init(&rb);
    rb.edge_loss = rb.prior_loss = loss;
    rb.edge_scale = rb.prior_scale = 3.;
    std::vector<double> out(static_cast<size_t>(n) * 16, -7.), ev(static_cast<size_t>(m) * 2, -7.), pv(static_cast<size_t>(k) * 2, -7.);
    lsa_pgo_result_t r;
    std::memset(&r, 0, sizeof(r));
    CHECK(lsa_pgo_solve_robust_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, lap.mask.data(), k ? lap.priors.data() : nullptr, k, lap.offset, nullptr, &rb,
                                    out.data(), &r, ev.data(), k ? pv.data() : nullptr) == LSA_OK);
    CHECK(AllFinite(out) && AllFinite(ev) && AllFinite(pv));
    CHECK(r.termination == LSA_PGO_STEP || r.termination == LSA_PGO_COST || r.termination == LSA_PGO_GRADIENT);
    CHECK(r.final_cost < r.initial_cost);
    for (int a = 0; a < n - 1; ++a) CHECK(ev[2 * static_cast<size_t>(a) + 1] == 1.);  // the chain is not robustified
    const double wFalse = ev[2 * static_cast<size_t>(lap.falseEdge) + 1], wTrue = ev[2 * static_cast<size_t>(lap.trueEdge) + 1];
    if (loss == LSA_PGO_LOSS_NONE)
    {
      CHECK(wFalse == 1. && wTrue == 1.);
      CHECK(std::memcmp(out.data(), plain.data(), out.size() * sizeof(double)) == 0);  // no loss: the solve as it was
      CHECK(r.final_cost == r0.final_cost && r.iterations == r0.iterations);
    }
    else
    {
      CHECK(wFalse < 0.05 && wTrue > 0.9);
      if (loss == LSA_PGO_LOSS_TUKEY) CHECK(wFalse == 0.);
      if (k) CHECK(pv[2 * static_cast<size_t>(lap.outlier) + 1] < 0.05 && pv[1] > 0.9);
    }
    // the verdicts are the linearization at the returned poses
    std::vector<double> e(static_cast<size_t>(m) * 6), blocks(static_cast<size_t>(m) * pg::kEdgeBlock), chi2(static_cast<size_t>(m)), rho(chi2.size()), w(chi2.size());
    CHECK(lsa_pgo_linearize_robust_host(out.data(), n, lap.edges.data(), m, lap.mask.data(), &rb, e.data(), blocks.data(), chi2.data(), rho.data(), w.data()) == LSA_OK);
    for (int a = 0; a < m; ++a) CHECK(chi2[static_cast<size_t>(a)] == ev[2 * static_cast<size_t>(a)] && w[static_cast<size_t>(a)] == ev[2 * static_cast<size_t>(a) + 1]);
    // every edge under the loss (mask NULL), no verdict asked for, in place
    std::vector<double> inplace = lap.poses;
    CHECK(lsa_pgo_solve_robust_host(inplace.data(), n, lap.fixed.data(), lap.edges.data(), m, nullptr, k ? lap.priors.data() : nullptr, k, lap.offset, nullptr, &rb, inplace.data(),
                                    &r, nullptr, nullptr) == LSA_OK);
    CHECK(AllFinite(inplace));
    // weighted records are the plain ones times the weight
    std::vector<double> b0(blocks.size()), c0(chi2.size()), e0(e.size());
    CHECK(lsa_pgo_linearize_host(out.data(), n, lap.edges.data(), m, e0.data(), b0.data(), c0.data()) == LSA_OK);
    for (int a = 0; a < m; ++a)
      for (int t = 0; t < pg::kEdgeBlock; ++t)
        CHECK(blocks[static_cast<size_t>(a) * pg::kEdgeBlock + t] == w[static_cast<size_t>(a)] * b0[static_cast<size_t>(a) * pg::kEdgeBlock + t]);
    if (k)
    {
      std::vector<double> pe(static_cast<size_t>(k) * 3), pb(static_cast<size_t>(k) * pg::kPriorBlock), pc(static_cast<size_t>(k)), pr(pc.size()), pw(pc.size());
      CHECK(lsa_pgo_linearize_robust_priors_host(out.data(), n, lap.priors.data(), k, lap.offset, &rb, pe.data(), pb.data(), pc.data(), pr.data(), pw.data()) == LSA_OK);
      for (int a = 0; a < k; ++a) CHECK(pc[static_cast<size_t>(a)] == pv[2 * static_cast<size_t>(a)] && pw[static_cast<size_t>(a)] == pv[2 * static_cast<size_t>(a) + 1]);
    }
  }
}

static void Refusals()
{
  const Lap lap = MakeLap(16, true);
  const int n = lap.n, m = static_cast<int>(lap.edges.size()), k = static_cast<int>(lap.priors.size());
  std::vector<double> out(static_cast<size_t>(n) * 16, -7.), ev(static_cast<size_t>(m) * 2, -7.), pv(static_cast<size_t>(k) * 2, -7.);
  lsa_pgo_result_t r;
  std::memset(&r, 0, sizeof(r));
  r.iterations = -7;
  auto refused = [&](const lsa_pgo_robust_t& rb) {
    CHECK(lsa_pgo_solve_robust_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, lap.mask.data(), lap.priors.data(), k, lap.offset, nullptr, &rb, out.data(), &r,
                                    ev.data(), pv.data()) == LSA_E_ARG);
    for (double v : out) CHECK(v == -7.);
    for (double v : ev) CHECK(v == -7.);
    for (double v : pv) CHECK(v == -7.);
    CHECK(r.iterations == -7);
    std::vector<double> e(static_cast<size_t>(m) * 6, -7.), blocks(static_cast<size_t>(m) * pg::kEdgeBlock, -7.), chi2(static_cast<size_t>(m), -7.), rho(chi2), w(chi2);
    CHECK(lsa_pgo_linearize_robust_host(lap.poses.data(), n, lap.edges.data(), m, lap.mask.data(), &rb, e.data(), blocks.data(), chi2.data(), rho.data(), w.data()) == LSA_E_ARG);
    for (double v : blocks) CHECK(v == -7.);
  };
  lsa_pgo_robust_t rb;
  lsa_pgo_robust_init(&rb);
  rb.edge_loss = 4;
  refused(rb);
  rb.edge_loss = -1;
  refused(rb);
  lsa_pgo_robust_init(&rb);
  rb.prior_loss = LSA_PGO_LOSS_HUBER;
  rb.prior_scale = 0.;
  refused(rb);
  rb.prior_scale = std::numeric_limits<double>::quiet_NaN();
  refused(rb);
  lsa_pgo_robust_init(&rb);
  rb.edge_loss = LSA_PGO_LOSS_TUKEY;
  rb.edge_scale = std::numeric_limits<double>::infinity();
  refused(rb);
  // a scale is not looked at while its loss is NONE
  lsa_pgo_robust_init(&rb);
  rb.edge_scale = -1.;
  CHECK(lsa_pgo_solve_robust_host(lap.poses.data(), n, lap.fixed.data(), lap.edges.data(), m, lap.mask.data(), lap.priors.data(), k, lap.offset, nullptr, &rb, out.data(), &r,
                                  ev.data(), pv.data()) == LSA_OK);
  CHECK(AllFinite(out) && AllFinite(ev) && AllFinite(pv));
}

int main()
{
  LossValues();
  SolveUnderEveryLoss(false);
  SolveUnderEveryLoss(true);
  Refusals();
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
