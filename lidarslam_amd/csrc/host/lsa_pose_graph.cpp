// lsa_pose_graph.cpp -- see lsa_pose_graph.h.  The loop is the one written in ../lsa_pose_graph.h's comment.
#include "lsa_pose_graph.h"
#include <cmath>
#include <cstring>

namespace lsa
{
namespace host
{
namespace
{
bool all_finite(const double* v, int n)
{
  for (int i = 0; i < n; ++i)
    if (!pg::finite_d(v[i])) return false;
  return true;
}

// block Thomas, factored once: W_i = L_i S_{i-1}^-1, S_i = D_i - W_i U_{i-1} (S_0 = D_0), the Cholesky factors of the S_i kept
struct Thomas
{
  int n = 0;
  std::vector<pg::Chol6> S;
  std::vector<double> W;
  const double* U = nullptr;
  bool Factor(int n_, const double* D, const double* L, const double* U_)
  {
    n = n_;
    U = U_;
    S.resize(static_cast<size_t>(n));
    W.assign(static_cast<size_t>(n) * 36, 0.);
    double Si[36], WU[36];
    for (int i = 0; i < n; ++i)
    {
      std::memcpy(Si, D + 36 * static_cast<size_t>(i), sizeof(Si));
      if (i > 0)
      {
        double* Wi = &W[36 * static_cast<size_t>(i)];
        pg::chol6_right(S[static_cast<size_t>(i) - 1], L + 36 * static_cast<size_t>(i), Wi);
        pg::mul6(Wi, U + 36 * static_cast<size_t>(i - 1), WU);
        for (int k = 0; k < 36; ++k) Si[k] -= WU[k];
      }
      if (!pg::chol6(Si, S[static_cast<size_t>(i)])) return false;
    }
    return true;
  }
  void Solve(const double* b, double* x) const
  {
    std::vector<double> y(static_cast<size_t>(n) * 6);
    double t[6];
    for (int i = 0; i < n; ++i)
    {
      double* yi = &y[6 * static_cast<size_t>(i)];
      for (int k = 0; k < 6; ++k) yi[k] = b[6 * static_cast<size_t>(i) + k];
      if (i > 0)
      {
        pg::mulv6(&W[36 * static_cast<size_t>(i)], yi - 6, t);
        for (int k = 0; k < 6; ++k) yi[k] -= t[k];
      }
    }
    for (int i = n - 1; i >= 0; --i)
    {
      double rhs[6];
      for (int k = 0; k < 6; ++k) rhs[k] = y[6 * static_cast<size_t>(i) + k];
      if (i + 1 < n)
      {
        pg::mulv6(U + 36 * static_cast<size_t>(i), x + 6 * static_cast<size_t>(i + 1), t);
        for (int k = 0; k < 6; ++k) rhs[k] -= t[k];
      }
      pg::chol6_solve(S[static_cast<size_t>(i)], rhs, x + 6 * static_cast<size_t>(i));
    }
  }
};

double Dot(const std::vector<double>& a, const std::vector<double>& b)
{
  double s = 0.;
  for (size_t i = 0; i < a.size(); ++i) s += a[i] * b[i];
  return s;
}

// the losses of a solve and the edges they act on
struct Robust
{
  lsa_pgo_robust_t r{LSA_PGO_LOSS_NONE, LSA_PGO_LOSS_NONE, 1., 1.};
  const unsigned char* mask = nullptr;  // NULL: every edge
  int EdgeLoss(int k) const { return (!mask || mask[k]) ? r.edge_loss : LSA_PGO_LOSS_NONE; }
};

struct System
{
  std::vector<double> e, blocks, chi2, rho, w, pe, pblocks, D, dg, g, L, U;  // chi2, rho, w: the m edge values, then the k prior values
  void Size(int n, int m, int k = 0)
  {
    rho.resize(static_cast<size_t>(m) + static_cast<size_t>(k));
    w.resize(rho.size());
    e.resize(static_cast<size_t>(m) * 6);
    blocks.resize(static_cast<size_t>(m) * pg::kEdgeBlock);
    chi2.resize(static_cast<size_t>(m) + static_cast<size_t>(k));
    pe.resize(static_cast<size_t>(k) * 3);
    pblocks.resize(static_cast<size_t>(k) * pg::kPriorBlock);
    D.resize(static_cast<size_t>(n) * 36);
    L.resize(D.size());
    U.resize(D.size());
    dg.resize(static_cast<size_t>(n) * 6);
    g.resize(dg.size());
  }
  // F = 1/2 sum rho; a constraint that is not robustified goes through the plain functions (rho = chi2, w = 1)
  double Linearize(const double* poses, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors = nullptr, int np = 0, const pg::Pose* O = nullptr,
                   const Robust& rb = Robust())
  {
    double F = 0.;
    for (int k = 0; k < m; ++k)
    {
      const size_t at = static_cast<size_t>(k);
      double* blk = &blocks[at * pg::kEdgeBlock];
      if (rb.EdgeLoss(k) == LSA_PGO_LOSS_NONE)
      {
        pg::linearize_edge(poses, edges[k], &e[6 * at], blk, &chi2[at]);
        rho[at] = chi2[at];
        w[at] = 1.;
      }
      else
        pg::linearize_edge_robust(poses, edges[k], rb.r.edge_loss, rb.r.edge_scale, &e[6 * at], blk, &chi2[at], &rho[at], &w[at]);
      F += rho[at];
    }
    for (int k = 0; k < np; ++k)
    {
      const size_t at = static_cast<size_t>(m) + static_cast<size_t>(k);
      double* blk = &pblocks[static_cast<size_t>(k) * pg::kPriorBlock];
      if (rb.r.prior_loss == LSA_PGO_LOSS_NONE)
      {
        pg::linearize_prior(poses, priors[k], *O, &pe[3 * static_cast<size_t>(k)], blk, &chi2[at]);
        rho[at] = chi2[at];
        w[at] = 1.;
      }
      else
        pg::linearize_prior_robust(poses, priors[k], *O, rb.r.prior_loss, rb.r.prior_scale, &pe[3 * static_cast<size_t>(k)], blk, &chi2[at], &rho[at], &w[at]);
      F += rho[at];
    }
    return 0.5 * F;
  }
  void Assemble(const PoseGraph& G, const unsigned char* fixed, const lsa_pgo_edge_t* edges, double lambda)
  {
    const pg::Graph v = G.view();
    for (int i = 0; i < G.n; ++i)
    {
      const size_t b = 36 * static_cast<size_t>(i), c = 6 * static_cast<size_t>(i);
      pg::assemble_row(i, G.n, fixed, v, edges, blocks.data(), pblocks.data(), lambda, &D[b], &dg[c], &g[c], &L[b], &U[b]);
    }
  }
};
}  // namespace

const char* PgoMessage(int termination)
{
  switch (termination)
  {
    case LSA_PGO_MAX_ITERATIONS: return "the maximum number of iterations was reached";
    case LSA_PGO_GRADIENT: return "the gradient is below its tolerance";
    case LSA_PGO_STEP: return "the step is below its tolerance";
    case LSA_PGO_COST: return "the relative decrease of the cost is below its tolerance";
    case LSA_PGO_LAMBDA_CEILING: return "the damping rose above its ceiling";
    case LSA_PGO_LINEAR_SOLVER_FAILED: return "the linear solver failed (a block is not positive definite)";
  }
  return "";
}

int PgoCheckEdges(const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, std::string* why)
{
  auto no = [&](const std::string& w) {
    if (why) *why = w;
    return LSA_E_ARG;
  };
  if (!poses16 || n < 1 || m < 0 || (m > 0 && !edges)) return no("bad argument");
  if (!all_finite(poses16, 16 * n)) return no("a pose has a non-finite entry");
  for (int k = 0; k < m; ++k)
  {
    const lsa_pgo_edge_t& ed = edges[k];
    if (ed.from < 0 || ed.from >= n || ed.to < 0 || ed.to >= n) return no("edge " + std::to_string(k) + " names a pose outside 0.." + std::to_string(n - 1));
    if (ed.from == ed.to) return no("edge " + std::to_string(k) + " joins a pose with itself");
    if (!all_finite(ed.relative, 16) || !all_finite(ed.information, 36)) return no("edge " + std::to_string(k) + " has a non-finite entry");
  }
  return LSA_OK;
}

int PgoCheckPriors(const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, std::string* why)
{
  auto no = [&](const std::string& w) {
    if (why) *why = w;
    return LSA_E_ARG;
  };
  if (!poses16 || n < 1 || k < 0 || (k > 0 && (!priors || !offset16))) return no("bad argument");
  if (k == 0) return LSA_OK;
  if (!all_finite(poses16, 16 * n)) return no("a pose has a non-finite entry");
  if (!all_finite(offset16, 16)) return no("the priors' offset has a non-finite entry");
  for (int a = 0; a < k; ++a)
  {
    if (priors[a].pose < 0 || priors[a].pose >= n) return no("prior " + std::to_string(a) + " names a pose outside 0.." + std::to_string(n - 1));
    if (!all_finite(priors[a].position, 3) || !all_finite(priors[a].information, 9)) return no("prior " + std::to_string(a) + " has a non-finite entry");
  }
  return LSA_OK;
}

int PgoBuild(const double* poses16, int n, const unsigned char* fixed, const lsa_pgo_edge_t* edges, int m, PoseGraph* g, std::string* why, const lsa_pgo_prior_t* priors,
             int np, const double* offset16)
{
  if (const int rc = PgoCheckEdges(poses16, n, edges, m, why); rc != LSA_OK) return rc;
  if (const int rc = PgoCheckPriors(poses16, n, priors, np, offset16, why); rc != LSA_OK) return rc;
  auto no = [&](const std::string& w) {
    if (why) *why = w;
    return LSA_E_ARG;
  };
  if (!fixed) return no("bad argument");
  bool anyFixed = false;
  for (int i = 0; i < n; ++i) anyFixed = anyFixed || fixed[i] != 0;
  if (!anyFixed && np == 0) return no("no pose is fixed and there is no prior");
  g->n = n;
  g->m = m;
  g->k = np;
  g->prior_start.assign(static_cast<size_t>(n) + 1, 0);
  for (int a = 0; a < np; ++a) ++g->prior_start[static_cast<size_t>(priors[a].pose) + 1];
  for (int i = 0; i < n; ++i) g->prior_start[static_cast<size_t>(i) + 1] += g->prior_start[static_cast<size_t>(i)];
  g->prior_of.assign(static_cast<size_t>(np), 0);
  {
    std::vector<int> pat(g->prior_start.begin(), g->prior_start.end() - 1);
    for (int a = 0; a < np; ++a) g->prior_of[static_cast<size_t>(pat[static_cast<size_t>(priors[a].pose)]++)] = a;
  }
  g->row_start.assign(static_cast<size_t>(n) + 1, 0);
  g->loop_start.assign(static_cast<size_t>(n) + 1, 0);
  auto beyond = [&](int a, int b) { return !fixed[a] && !fixed[b] && a - b != 1 && b - a != 1; };
  for (int k = 0; k < m; ++k)
  {
    ++g->row_start[static_cast<size_t>(edges[k].from) + 1];
    ++g->row_start[static_cast<size_t>(edges[k].to) + 1];
    if (beyond(edges[k].from, edges[k].to))
    {
      ++g->loop_start[static_cast<size_t>(edges[k].from) + 1];
      ++g->loop_start[static_cast<size_t>(edges[k].to) + 1];
    }
  }
  for (int i = 0; i < n; ++i)
  {
    if (!fixed[i] && g->row_start[static_cast<size_t>(i) + 1] == 0) return no("free pose " + std::to_string(i) + " has no edge");
    g->row_start[static_cast<size_t>(i) + 1] += g->row_start[static_cast<size_t>(i)];
    g->loop_start[static_cast<size_t>(i) + 1] += g->loop_start[static_cast<size_t>(i)];
  }
  g->inc.assign(static_cast<size_t>(2) * m, 0);
  g->loop_edge.assign(static_cast<size_t>(g->loop_start[static_cast<size_t>(n)]), 0);
  g->loop_col.assign(g->loop_edge.size(), 0);
  std::vector<int> at(g->row_start.begin(), g->row_start.end() - 1), lat(g->loop_start.begin(), g->loop_start.end() - 1);
  for (int k = 0; k < m; ++k)
  {
    const int a = edges[k].from, b = edges[k].to;
    g->inc[static_cast<size_t>(at[static_cast<size_t>(a)]++)] = k;
    g->inc[static_cast<size_t>(at[static_cast<size_t>(b)]++)] = k;
    if (beyond(a, b))
    {
      g->loop_edge[static_cast<size_t>(lat[static_cast<size_t>(a)])] = 2 * k;
      g->loop_col[static_cast<size_t>(lat[static_cast<size_t>(a)]++)] = b;
      g->loop_edge[static_cast<size_t>(lat[static_cast<size_t>(b)])] = 2 * k + 1;
      g->loop_col[static_cast<size_t>(lat[static_cast<size_t>(b)]++)] = a;
    }
  }
  return LSA_OK;
}

bool PgoTridiagonalSolve(int n, const double* D, const double* L, const double* U, const double* b, double* x)
{
  Thomas t;
  if (!t.Factor(n, D, L, U)) return false;
  std::vector<double> y(static_cast<size_t>(n) * 6);
  t.Solve(b, y.data());
  if (!all_finite(y.data(), 6 * n)) return false;
  std::memcpy(x, y.data(), y.size() * sizeof(double));
  return true;
}

int PgoSolve(const double* poses16, int n, const unsigned char* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int np, const double* offset16,
             const lsa_pgo_params_t* params, double* poses_out, lsa_pgo_result_t* result, std::string* why, const unsigned char* edgeMask, const lsa_pgo_robust_t* robust,
             double* edgeVerdict, double* priorVerdict)
{
  lsa_pgo_params_t p;
  lsa_pgo_params_init(&p);
  if (params) p = *params;
  Robust rb;
  rb.mask = edgeMask;
  if (robust) rb.r = *robust;
  if (!poses_out || !result || !pg::params_ok(p) || !pg::robust_ok(rb.r))
  {
    if (why) *why = "bad argument or parameters out of limits";
    return LSA_E_ARG;
  }
  PoseGraph G;
  if (const int rc = PgoBuild(poses16, n, fixed, edges, m, &G, why, priors, np, offset16); rc != LSA_OK) return rc;
  const pg::Graph view = G.view();
  pg::Pose O = pg::load(poses16);  // unused without priors
  if (np > 0) O = pg::load(offset16);
  const size_t nv = static_cast<size_t>(n) * 6;
  std::vector<double> x(poses16, poses16 + 16 * static_cast<size_t>(n)), cand(x.size());
  System S;
  S.Size(n, m, np);
  std::vector<double> delta(nv), r(nv), z(nv), pv(nv), q(nv), zeros;
  lsa_pgo_result_t R;
  std::memset(&R, 0, sizeof(R));
  double F = S.Linearize(x.data(), edges, m, priors, np, &O, rb);
  R.initial_cost = F;
  double lambda = p.initial_lambda;
  int term = LSA_PGO_MAX_ITERATIONS;
  Thomas T;
  for (int it = 0; it < p.max_iterations; ++it)
  {
    R.iterations = it + 1;
    S.Assemble(G, fixed, edges, lambda);
    double gmax = 0.;
    for (size_t k = 0; k < nv; ++k) gmax = std::fabs(S.g[k]) > gmax ? std::fabs(S.g[k]) : gmax;
    if (gmax <= p.gradient_tolerance) { term = LSA_PGO_GRADIENT; break; }
    if (p.preconditioner == 1) zeros.assign(S.D.size(), 0.);
    const double* TL = p.preconditioner == 1 ? zeros.data() : S.L.data();
    const double* TU = p.preconditioner == 1 ? zeros.data() : S.U.data();
    if (!T.Factor(n, S.D.data(), TL, TU)) { term = LSA_PGO_LINEAR_SOLVER_FAILED; break; }
    // PCG
    bool failed = false;
    int iters = 0;
    for (size_t k = 0; k < nv; ++k) { delta[k] = 0.; r[k] = -S.g[k]; }
    T.Solve(r.data(), z.data());
    pv = z;
    double rz = Dot(r, z);
    const double rz0 = rz;
    bool converged = rz0 == 0.;
    if (!pg::finite_d(rz0) || rz0 < 0.) failed = true;
    while (!converged && !failed && iters < p.pcg_max_iter)
    {
      ++iters;
      for (int i = 0; i < n; ++i) pg::spmv_row(i, n, view, S.blocks.data(), S.D.data(), S.L.data(), S.U.data(), pv.data(), &q[6 * static_cast<size_t>(i)]);
      const double pq = Dot(pv, q);
      if (!(pq > 0.) || !pg::finite_d(pq)) { failed = true; break; }
      const double alpha = rz / pq;
      for (size_t k = 0; k < nv; ++k) { delta[k] += alpha * pv[k]; r[k] -= alpha * q[k]; }
      T.Solve(r.data(), z.data());
      const double rzn = Dot(r, z);
      if (!pg::finite_d(rzn)) { failed = true; break; }
      if (rzn <= p.pcg_tolerance * p.pcg_tolerance * rz0) { converged = true; break; }
      const double beta = rzn / rz;
      for (size_t k = 0; k < nv; ++k) pv[k] = z[k] + beta * pv[k];
      rz = rzn;
    }
    R.pcg_iterations += iters;
    R.last_pcg_iterations = iters;
    if (failed) { term = LSA_PGO_LINEAR_SOLVER_FAILED; break; }
    if (!converged) ++R.pcg_truncated;
    double step = 0., model = 0.;
    for (size_t k = 0; k < nv; ++k)
    {
      step = std::fabs(delta[k]) > step ? std::fabs(delta[k]) : step;
      model += delta[k] * (lambda * S.dg[k] * delta[k] - S.g[k]);
    }
    model *= 0.5;
    for (int i = 0; i < n; ++i) pg::store(pg::retract(pg::load(&x[16 * static_cast<size_t>(i)]), &delta[6 * static_cast<size_t>(i)]), &cand[16 * static_cast<size_t>(i)]);
    double Fn = 0.;
    double raw, wt;
    for (int k = 0; k < m; ++k) Fn += pg::edge_rho(cand.data(), edges[k], rb.EdgeLoss(k), rb.r.edge_scale, &raw, &wt);
    for (int k = 0; k < np; ++k) Fn += pg::prior_rho(cand.data(), priors[k], O, rb.r.prior_loss, rb.r.prior_scale, &raw, &wt);
    Fn *= 0.5;
    if (model > 0. && pg::finite_d(Fn) && F - Fn > 0.)
    {
      const double dec = F - Fn;
      x = cand;
      const bool small = dec <= p.cost_tolerance * F;
      F = S.Linearize(x.data(), edges, m, priors, np, &O, rb);
      ++R.accepted_steps;
      R.largest_step = step > R.largest_step ? step : R.largest_step;
      lambda = lambda * p.lambda_shrink > p.lambda_min ? lambda * p.lambda_shrink : p.lambda_min;
      if (step <= p.step_tolerance) { term = LSA_PGO_STEP; break; }
      if (small) { term = LSA_PGO_COST; break; }
    }
    else
    {
      ++R.rejected_steps;
      lambda *= p.lambda_grow;
      if (step <= p.step_tolerance) { term = LSA_PGO_STEP; break; }
      if (lambda > p.lambda_max) { term = LSA_PGO_LAMBDA_CEILING; break; }
    }
  }
  R.final_cost = F;
  R.final_lambda = lambda;
  R.termination = term;
  R.message = PgoMessage(term);
  // the verdicts: one more evaluation at the returned poses
  for (int k = 0; edgeVerdict && k < m; ++k) (void)pg::edge_rho(x.data(), edges[k], rb.EdgeLoss(k), rb.r.edge_scale, edgeVerdict + 2 * static_cast<size_t>(k), edgeVerdict + 2 * static_cast<size_t>(k) + 1);
  for (int k = 0; priorVerdict && k < np; ++k)
    (void)pg::prior_rho(x.data(), priors[k], O, rb.r.prior_loss, rb.r.prior_scale, priorVerdict + 2 * static_cast<size_t>(k), priorVerdict + 2 * static_cast<size_t>(k) + 1);
  std::memcpy(poses_out, x.data(), x.size() * sizeof(double));
  *result = R;
  return LSA_OK;
}
}  // namespace host
}  // namespace lsa

using namespace lsa;

extern "C" {

void lsa_pgo_params_init(lsa_pgo_params_t* p)
{
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = 50;
  p->pcg_max_iter = 500;
  p->pcg_tolerance = 1e-8;
  p->initial_lambda = 1e-6;
  p->lambda_shrink = 0.25;
  p->lambda_grow = 8.;
  p->lambda_min = 1e-12;
  p->lambda_max = 1e12;
  p->gradient_tolerance = 1e-12;
  p->step_tolerance = 1e-10;
  p->cost_tolerance = 1e-13;
  for (int k = 0; k < 6; ++k) p->odometry_sigma[k] = k < 3 ? 0.05 : 0.01;
}

int lsa_pgo_solve_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_params_t* params, double* poses_out,
                       lsa_pgo_result_t* result)
{
  return lsa_pgo_solve_priors_host(poses16, n, fixed, edges, m, nullptr, 0, nullptr, params, poses_out, result);
}

int lsa_pgo_solve_priors_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                              const double* offset16, const lsa_pgo_params_t* params, double* poses_out, lsa_pgo_result_t* result)
{
  return lsa_pgo_solve_robust_host(poses16, n, fixed, edges, m, nullptr, priors, k, offset16, params, nullptr, poses_out, result, nullptr, nullptr);
}

void lsa_pgo_robust_init(lsa_pgo_robust_t* r)
{
  if (!r) return;
  std::memset(r, 0, sizeof(*r));
  r->edge_loss = LSA_PGO_LOSS_NONE;
  r->prior_loss = LSA_PGO_LOSS_NONE;
  r->edge_scale = 1.;
  r->prior_scale = 1.;
}

int lsa_pgo_robust_rho_host(int loss, double scale, double s, double* rho_out, double* w_out)
{
  lsa_pgo_robust_t r;
  lsa_pgo_robust_init(&r);
  r.edge_loss = loss;
  r.edge_scale = scale;
  if (!rho_out || !w_out || !pg::robust_ok(r)) return LSA_E_ARG;
  pg::robust_rho(loss, scale, s, rho_out, w_out);
  return LSA_OK;
}

int lsa_pgo_solve_robust_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask, const lsa_pgo_prior_t* priors,
                              int k, const double* offset16, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust, double* poses_out, lsa_pgo_result_t* result,
                              double* edge_verdict_out, double* prior_verdict_out)
{
  return host::PgoSolve(poses16, n, fixed, edges, m, priors, k, offset16, params, poses_out, result, nullptr, edge_mask, robust, edge_verdict_out, prior_verdict_out);
}

int lsa_pgo_linearize_robust_host(const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask, const lsa_pgo_robust_t* robust, double* e_out,
                                  double* blocks_out, double* chi2_out, double* rho_out, double* w_out)
{
  host::Robust rb;
  rb.mask = edge_mask;
  if (robust) rb.r = *robust;
  if (!e_out || !blocks_out || !chi2_out || !rho_out || !w_out || !pg::robust_ok(rb.r)) return LSA_E_ARG;
  if (const int rc = host::PgoCheckEdges(poses16, n, edges, m, nullptr); rc != LSA_OK) return rc;
  for (int a = 0; a < m; ++a)
    pg::linearize_edge_robust(poses16, edges[a], rb.EdgeLoss(a), rb.r.edge_scale, e_out + 6 * static_cast<size_t>(a), blocks_out + static_cast<size_t>(a) * pg::kEdgeBlock,
                              chi2_out + a, rho_out + a, w_out + a);
  return LSA_OK;
}

int lsa_pgo_linearize_robust_priors_host(const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, const lsa_pgo_robust_t* robust,
                                         double* e_out, double* blocks_out, double* chi2_out, double* rho_out, double* w_out)
{
  host::Robust rb;
  if (robust) rb.r = *robust;
  if (!e_out || !blocks_out || !chi2_out || !rho_out || !w_out || !pg::robust_ok(rb.r)) return LSA_E_ARG;
  if (const int rc = host::PgoCheckPriors(poses16, n, priors, k, offset16, nullptr); rc != LSA_OK) return rc;
  if (k == 0) return LSA_OK;
  const pg::Pose O = pg::load(offset16);
  for (int a = 0; a < k; ++a)
    pg::linearize_prior_robust(poses16, priors[a], O, rb.r.prior_loss, rb.r.prior_scale, e_out + 3 * static_cast<size_t>(a),
                               blocks_out + static_cast<size_t>(a) * pg::kPriorBlock, chi2_out + a, rho_out + a, w_out + a);
  return LSA_OK;
}

int lsa_pgo_linearize_priors_host(const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, double* e_out, double* blocks_out,
                                  double* chi2_out)
{
  if (!e_out || !blocks_out || !chi2_out) return LSA_E_ARG;
  if (const int rc = host::PgoCheckPriors(poses16, n, priors, k, offset16, nullptr); rc != LSA_OK) return rc;
  if (k == 0) return LSA_OK;
  const pg::Pose O = pg::load(offset16);
  for (int a = 0; a < k; ++a) pg::linearize_prior(poses16, priors[a], O, e_out + 3 * static_cast<size_t>(a), blocks_out + static_cast<size_t>(a) * pg::kPriorBlock, chi2_out + a);
  return LSA_OK;
}

int lsa_pgo_prior_jacobian_host(const double* poses16, int n, const lsa_pgo_prior_t* prior, const double* offset16, double* e3, double* A18)
{
  if (!e3 || !A18 || !prior) return LSA_E_ARG;
  if (const int rc = host::PgoCheckPriors(poses16, n, prior, 1, offset16, nullptr); rc != LSA_OK) return rc;
  pg::prior_eval(pg::load(poses16 + 16 * static_cast<size_t>(prior->pose)), pg::load(offset16), prior->position, e3, A18);
  return LSA_OK;
}

int lsa_pgo_premultiply_host(const double* poses16, int n, const double* W16, double* poses_out)
{
  if (!poses16 || !W16 || !poses_out || n < 1) return LSA_E_ARG;
  const pg::Pose W = pg::load(W16);
  for (int i = 0; i < n; ++i) pg::store(pg::compose(W, pg::load(poses16 + 16 * static_cast<size_t>(i))), poses_out + 16 * static_cast<size_t>(i));
  return LSA_OK;
}

int lsa_pgo_reanchor_host(const double* poses16, int n, double* poses_out)
{
  if (!poses16 || !poses_out || n < 1) return LSA_E_ARG;
  const pg::Pose A = pg::load(poses16);  // read before pose 0 is written: poses_out may be poses16
  for (int i = 0; i < n; ++i) pg::store(pg::inverse_compose(A, pg::load(poses16 + 16 * static_cast<size_t>(i))), poses_out + 16 * static_cast<size_t>(i));
  return LSA_OK;
}

int lsa_pgo_linearize_host(const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, double* e_out, double* blocks_out, double* chi2_out)
{
  if (!e_out || !blocks_out || !chi2_out) return LSA_E_ARG;
  if (const int rc = host::PgoCheckEdges(poses16, n, edges, m, nullptr); rc != LSA_OK) return rc;
  for (int k = 0; k < m; ++k) pg::linearize_edge(poses16, edges[k], e_out + 6 * static_cast<size_t>(k), blocks_out + static_cast<size_t>(k) * pg::kEdgeBlock, chi2_out + k);
  return LSA_OK;
}

int lsa_pgo_assemble_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, double* D_out, double* g_out,
                          double* L_out, double* U_out)
{
  return lsa_pgo_assemble_priors_host(poses16, n, fixed, edges, m, nullptr, 0, nullptr, lambda, D_out, g_out, L_out, U_out);
}

int lsa_pgo_assemble_priors_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                                 const double* offset16, double lambda, double* D_out, double* g_out, double* L_out, double* U_out)
{
  if (!D_out || !g_out || !L_out || !U_out || !(lambda >= 0.) || !pg::finite_d(lambda)) return LSA_E_ARG;
  host::PoseGraph G;
  if (const int rc = host::PgoBuild(poses16, n, fixed, edges, m, &G, nullptr, priors, k, offset16); rc != LSA_OK) return rc;
  host::System S;
  S.Size(n, m, k);
  const pg::Pose O = pg::load(k > 0 ? offset16 : poses16);
  S.Linearize(poses16, edges, m, priors, k, &O);
  S.Assemble(G, fixed, edges, lambda);
  std::memcpy(D_out, S.D.data(), S.D.size() * sizeof(double));
  std::memcpy(g_out, S.g.data(), S.g.size() * sizeof(double));
  std::memcpy(L_out, S.L.data(), S.L.size() * sizeof(double));
  std::memcpy(U_out, S.U.data(), S.U.size() * sizeof(double));
  return LSA_OK;
}

int lsa_pgo_tridiagonal_solve_host(int n, const double* D, const double* L, const double* U, const double* b, double* x)
{
  if (n < 1 || !D || !L || !U || !b || !x) return LSA_E_ARG;
  return host::PgoTridiagonalSolve(n, D, L, U, b, x) ? LSA_OK : 1;
}

int lsa_pgo_spmv_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, const double* p, double* q)
{
  return lsa_pgo_spmv_priors_host(poses16, n, fixed, edges, m, nullptr, 0, nullptr, lambda, p, q);
}

int lsa_pgo_spmv_priors_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                             const double* offset16, double lambda, const double* p, double* q)
{
  if (!p || !q || !(lambda >= 0.) || !pg::finite_d(lambda)) return LSA_E_ARG;
  host::PoseGraph G;
  if (const int rc = host::PgoBuild(poses16, n, fixed, edges, m, &G, nullptr, priors, k, offset16); rc != LSA_OK) return rc;
  host::System S;
  S.Size(n, m, k);
  const pg::Pose O = pg::load(k > 0 ? offset16 : poses16);
  S.Linearize(poses16, edges, m, priors, k, &O);
  S.Assemble(G, fixed, edges, lambda);
  std::vector<double> out(static_cast<size_t>(n) * 6);
  const pg::Graph view = G.view();
  for (int i = 0; i < n; ++i) pg::spmv_row(i, n, view, S.blocks.data(), S.D.data(), S.L.data(), S.U.data(), p, &out[6 * static_cast<size_t>(i)]);
  std::memcpy(q, out.data(), out.size() * sizeof(double));
  return LSA_OK;
}

int lsa_pgo_retract_host(const double* poses16, int n, const double* delta, double* poses_out)
{
  if (!poses16 || !delta || !poses_out || n < 1) return LSA_E_ARG;
  for (int i = 0; i < n; ++i) pg::store(pg::retract(pg::load(poses16 + 16 * static_cast<size_t>(i)), delta + 6 * static_cast<size_t>(i)), poses_out + 16 * static_cast<size_t>(i));
  return LSA_OK;
}

int lsa_pgo_edge_jacobians_host(const double* poses16, int n, const lsa_pgo_edge_t* edge, double* e6, double* A36, double* B36)
{
  if (!e6 || !A36 || !B36) return LSA_E_ARG;
  if (const int rc = host::PgoCheckEdges(poses16, n, edge, 1, nullptr); rc != LSA_OK) return rc;
  pg::edge_eval(pg::load(poses16 + 16 * static_cast<size_t>(edge->from)), pg::load(poses16 + 16 * static_cast<size_t>(edge->to)), pg::load(edge->relative), e6, A36, B36);
  return LSA_OK;
}

int lsa_pgo_information_from_covariance(const double* cov36, double* info36)
{
  if (!cov36 || !info36) return LSA_E_ARG;
  for (int i = 0; i < 36; ++i)
    if (!pg::finite_d(cov36[i])) return LSA_E_ARG;
  // symmetric to rounding, or it is no covariance
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < i; ++j)
    {
      const double a = cov36[i * 6 + j], b = cov36[j * 6 + i];
      if (std::fabs(a - b) > 1e-9 * (std::fabs(a) + std::fabs(b))) return LSA_E_ARG;
    }
  pg::Chol6 c;
  if (!pg::chol6(cov36, c)) return LSA_E_ARG;
  // a pivot that rounding alone left positive: singular to working precision
  for (int i = 0; i < 6; ++i)
    if (!(c.L[i * 6 + i] * c.L[i * 6 + i] > 1e-12 * cov36[i * 6 + i])) return LSA_E_ARG;
  double out[36];
  for (int k = 0; k < 6; ++k)
  {
    double unit[6] = {0, 0, 0, 0, 0, 0}, col[6];
    unit[k] = 1.;
    pg::chol6_solve(c, unit, col);
    for (int i = 0; i < 6; ++i) out[i * 6 + k] = col[i];
  }
  for (int i = 0; i < 36; ++i)
    if (!pg::finite_d(out[i])) return LSA_E_ARG;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) info36[i * 6 + j] = info36[j * 6 + i] = 0.5 * (out[i * 6 + j] + out[j * 6 + i]);
  return LSA_OK;
}

int lsa_pgo_information_from_covariance3(const double* cov9, double* info9)
{
  if (!cov9 || !info9) return LSA_E_ARG;
  for (int i = 0; i < 9; ++i)
    if (!pg::finite_d(cov9[i])) return LSA_E_ARG;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < i; ++j)
    {
      const double a = cov9[i * 3 + j], b = cov9[j * 3 + i];
      if (std::fabs(a - b) > 1e-9 * (std::fabs(a) + std::fabs(b))) return LSA_E_ARG;
    }
  // Cholesky of the lower triangle; a pivot that rounding alone left positive is singular to working precision (as the 6x6 rule)
  double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, rinv[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j <= i; ++j)
    {
      double s = cov9[i * 3 + j];
      for (int k = 0; k < j; ++k) s -= L[i * 3 + k] * L[j * 3 + k];
      if (i == j)
      {
        if (!(s > 1e-12 * cov9[i * 4]) || !(s <= 1.79769313486231570815e308)) return LSA_E_ARG;
        L[i * 4] = std::sqrt(s);
        rinv[i] = 1.0 / L[i * 4];
      }
      else
        L[i * 3 + j] = s * rinv[j];
    }
  double out[9];
  for (int c = 0; c < 3; ++c)
  {
    double y[3], x[3];
    for (int i = 0; i < 3; ++i)
    {
      double s = i == c ? 1. : 0.;
      for (int k = 0; k < i; ++k) s -= L[i * 3 + k] * y[k];
      y[i] = s * rinv[i];
    }
    for (int i = 2; i >= 0; --i)
    {
      double s = y[i];
      for (int k = i + 1; k < 3; ++k) s -= L[k * 3 + i] * x[k];
      x[i] = s * rinv[i];
    }
    for (int i = 0; i < 3; ++i) out[i * 3 + c] = x[i];
  }
  for (int i = 0; i < 9; ++i)
    if (!pg::finite_d(out[i])) return LSA_E_ARG;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j <= i; ++j) info9[i * 3 + j] = info9[j * 3 + i] = 0.5 * (out[i * 3 + j] + out[j * 3 + i]);
  return LSA_OK;
}

}  // extern "C"
