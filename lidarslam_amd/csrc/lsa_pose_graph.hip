// lsa_pose_graph.hip -- the pose-graph solve on the device.  The definition -- error, Jacobians, the order of
// every sum, the LM loop -- is lsa_pose_graph.h, the text the host statement (host/lsa_pose_graph.cpp) compiles too; the kernels
// below decide only who computes what.  All double precision, no floating-point atomics, every sum in a fixed order: two runs
// give the same bits.  No kernel waits for the host or for another workgroup; every launch is finite whatever the data.
//   k_pgo_linearize   a thread per edge: e, A, B, the edge's block record, chi2
//   k_pgo_linearize_priors   a thread per position prior: e, the prior's block record, chi2 behind the edges' values
//   k_pgo_assemble    a thread per pose: walks its incidence list ascending, then its priors; D (damped), diag(H), g, the
//                     tridiagonal L / U
//   k_pgo_pcr_level   block parallel cyclic reduction of the preconditioner T, one launch per stride s = 1, 2, 4, .. < n, a
//                     thread per row: alpha = -L_i D_{i-s}^-1, gamma = -U_i D_{i+s}^-1, D' = D + alpha U_{i-s} + gamma L_{i+s},
//                     L' = alpha L_{i-s}, U' = gamma U_{i+s}; alpha and gamma of every level are KEPT, so that an application
//                     of T^-1 is ceil(log2 n) light launches (k_pgo_pcr_apply) plus one (k_pgo_pcr_solve with the inverses
//                     of the last level's diagonal blocks).  36 n doubles twice per level: 262144 poses is the limit
//                     (LSA_E_CAPACITY), 2.7 GB there.  A block that is not positive definite raises a flag.
//   k_pgo_spmv        row i = D_i p_i + L_i p_{i-1} + U_i p_{i+1} + the blocks beyond the chain in the order of the row's list,
//                     and the workgroup's partial sum of p.q
//   PCG's vector updates and dot products: a partial sum per workgroup by a fixed tree, the partial sums added in order by
//   one thread, which also forms alpha and beta -- they stay on the device; the host reads one status block per iteration
//   to decide whether to enqueue the next.
//   k_pgo_retract, k_pgo_chi2, k_pgo_chi2_priors and the sums for the candidate.
//   k_pgo_linearize_robust, k_pgo_linearize_priors_robust, k_pgo_chi2_robust, k_pgo_chi2_priors_robust   the four kernels of the
//                     constraints under robust losses, launched in place of them when a loss is set: no launch
//                     is added to an LM iteration.  The verdicts are one more launch of the chi2 pair after the loop.
//   k_pgo_premultiply, k_pgo_reanchor   a thread per pose: W P_i, and inv(P_0) P_i (a trajectory into the frame of the measured
//                     positions and back onto its first pose).
// Buffers belong to the context and grow through its graveyard; everything runs on the context's stream.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "lsa_ctx.h"
#include "lsa_pose_graph.h"
#include "host/lsa_pose_graph.h"

using namespace lsa;

namespace lsa
{
struct PgoState
{
  double rz, rz0, pq, alpha, beta;
  double stat[4];  // model decrease, max |delta|, max |g|, sum of chi2
  int iters, converged, failed, notspd;
};
struct PgoBuf
{
  void* p = nullptr;
  size_t cap = 0;
};
struct PgoBuffers
{
  PgoBuf poses, cand, edges, fixed, row_start, inc, loop_start, loop_edge, loop_col, e, blocks, chi2, D, dg, g, L, U, work[2], alpha, gamma, Dinv, vec, partials, state, priors, prior_start, prior_of,
      pe, pblocks, mask, cost, weight, verdict;
  PgoState* host = nullptr;  // pinned
};
void pgo_destroy(lsa_ctx* ctx)
{
  PgoBuffers* b = ctx->pgo;
  if (!b) return;
  PgoBuf* all[] = {&b->poses, &b->cand, &b->edges, &b->fixed, &b->row_start, &b->inc, &b->loop_start, &b->loop_edge, &b->loop_col, &b->e, &b->blocks, &b->chi2, &b->D,
                   &b->dg, &b->g, &b->L, &b->U, &b->work[0], &b->work[1], &b->alpha, &b->gamma, &b->Dinv, &b->vec, &b->partials, &b->state, &b->priors, &b->prior_start,
                   &b->prior_of, &b->pe, &b->pblocks, &b->mask, &b->cost, &b->weight, &b->verdict};
  for (PgoBuf* x : all)
    if (x->p) (void)hipFree(x->p);
  if (b->host) (void)hipHostFree(b->host);
  delete b;
  ctx->pgo = nullptr;
}
}  // namespace lsa

namespace
{
constexpr int kThreads = 256;
constexpr int kMaxPoses = 262144;
inline unsigned blocks_for(long long n) { return (unsigned)std::max<long long>(1, (n + kThreads - 1) / kThreads); }

__global__ __launch_bounds__(kThreads) void k_pgo_linearize(const double* __restrict__ poses, const lsa_pgo_edge_t* __restrict__ edges, int m, double* __restrict__ e,
                                                            double* __restrict__ blocks, double* __restrict__ chi2)
{
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= m) return;
  pg::linearize_edge(poses, edges[k], e + 6LL * k, blocks + (long long)k * pg::kEdgeBlock, chi2 + k);
}

__global__ __launch_bounds__(kThreads) void k_pgo_chi2(const double* __restrict__ poses, const lsa_pgo_edge_t* __restrict__ edges, int m, double* __restrict__ chi2)
{
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= m) return;
  chi2[k] = pg::edge_chi2(poses, edges[k]);
}

// the priors' values go behind the m edge values of chi2
__global__ __launch_bounds__(kThreads) void k_pgo_linearize_priors(const double* __restrict__ poses, const lsa_pgo_prior_t* __restrict__ priors, int k, pg::Pose O,
                                                                   double* __restrict__ e, double* __restrict__ blocks, double* __restrict__ chi2)
{
  const int a = blockIdx.x * kThreads + threadIdx.x;
  if (a >= k) return;
  pg::linearize_prior(poses, priors[a], O, e + 3LL * a, blocks + (long long)a * pg::kPriorBlock, chi2 + a);
}

__global__ __launch_bounds__(kThreads) void k_pgo_chi2_priors(const double* __restrict__ poses, const lsa_pgo_prior_t* __restrict__ priors, int k, pg::Pose O,
                                                              double* __restrict__ chi2)
{
  const int a = blockIdx.x * kThreads + threadIdx.x;
  if (a >= k) return;
  chi2[a] = pg::prior_chi2(poses, priors[a], O);
}

// The four kernels above under losses (lsa_pose_graph.h ROBUST LOSS): the variants a solve launches IN PLACE of them when a loss
// is set, so a solve without one runs the kernels above untouched.  `cost` and `weight` hold the m edge values and then the k
// prior values, as chi2 does; the cost is summed from `cost`.
struct PgoLoss
{
  int edge_loss, prior_loss;
  double edge_scale, prior_scale;
  const unsigned char* mask;  // NULL: every edge
};
__device__ inline int edge_loss_of(const PgoLoss& loss, int k) { return (!loss.mask || loss.mask[k]) ? loss.edge_loss : LSA_PGO_LOSS_NONE; }

// the weight scales each element of the record as its sum leaves the registers: the record is written once, never read back
__global__ __launch_bounds__(kThreads) void k_pgo_linearize_robust(const double* __restrict__ poses, const lsa_pgo_edge_t* __restrict__ edges, int m, PgoLoss loss,
                                                                   double* __restrict__ e, double* __restrict__ blocks, double* __restrict__ chi2,
                                                                   double* __restrict__ cost, double* __restrict__ weight)
{
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= m) return;
  pg::linearize_edge_robust(poses, edges[k], edge_loss_of(loss, k), loss.edge_scale, e + 6LL * k, blocks + (long long)k * pg::kEdgeBlock, chi2 + k, cost + k, weight + k);
}
__global__ __launch_bounds__(kThreads) void k_pgo_linearize_priors_robust(const double* __restrict__ poses, const lsa_pgo_prior_t* __restrict__ priors, int k, pg::Pose O,
                                                                          PgoLoss loss, double* __restrict__ e, double* __restrict__ blocks, double* __restrict__ chi2,
                                                                          double* __restrict__ cost, double* __restrict__ weight)
{
  const int a = blockIdx.x * kThreads + threadIdx.x;
  if (a >= k) return;
  pg::linearize_prior_robust(poses, priors[a], O, loss.prior_loss, loss.prior_scale, e + 3LL * a, blocks + (long long)a * pg::kPriorBlock, chi2 + a, cost + a, weight + a);
}
// VERDICT false: out[k] = rho (a candidate's cost values); true: out[2 k] = chi2, out[2 k + 1] = w (the verdicts after the loop)
template <bool VERDICT>
__global__ __launch_bounds__(kThreads) void k_pgo_chi2_robust(const double* __restrict__ poses, const lsa_pgo_edge_t* __restrict__ edges, int m, PgoLoss loss,
                                                              double* __restrict__ out)
{
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= m) return;
  double s, w;
  const double rho = pg::edge_rho(poses, edges[k], edge_loss_of(loss, k), loss.edge_scale, &s, &w);
  if constexpr (VERDICT)
  {
    out[2LL * k] = s;
    out[2LL * k + 1] = w;
  }
  else
    out[k] = rho;
}
template <bool VERDICT>
__global__ __launch_bounds__(kThreads) void k_pgo_chi2_priors_robust(const double* __restrict__ poses, const lsa_pgo_prior_t* __restrict__ priors, int k, pg::Pose O,
                                                                     PgoLoss loss, double* __restrict__ out)
{
  const int a = blockIdx.x * kThreads + threadIdx.x;
  if (a >= k) return;
  double s, w;
  const double rho = pg::prior_rho(poses, priors[a], O, loss.prior_loss, loss.prior_scale, &s, &w);
  if constexpr (VERDICT)
  {
    out[2LL * a] = s;
    out[2LL * a + 1] = w;
  }
  else
    out[a] = rho;
}

__global__ __launch_bounds__(kThreads) void k_pgo_assemble(int n, const unsigned char* __restrict__ fixed, pg::Graph G, const lsa_pgo_edge_t* __restrict__ edges,
                                                           const double* __restrict__ blocks, const double* __restrict__ pblocks, double lambda, double* __restrict__ D,
                                                           double* __restrict__ dg, double* __restrict__ g, double* __restrict__ L, double* __restrict__ U)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  pg::assemble_row(i, n, fixed, G, edges, blocks, pblocks, lambda, D + 36LL * i, dg + 6LL * i, g + 6LL * i, L + 36LL * i, U + 36LL * i);
}

// one level of the cyclic reduction at stride s
__global__ __launch_bounds__(kThreads) void k_pgo_pcr_level(int n, int s, const double* __restrict__ Din, const double* __restrict__ Lin, const double* __restrict__ Uin,
                                                            double* __restrict__ Dout, double* __restrict__ Lout, double* __restrict__ Uout, double* __restrict__ alpha,
                                                            double* __restrict__ gamma, PgoState* st)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const long long at = 36LL * i;
  double Dn[36], X[36], T[36];
  for (int k = 0; k < 36; ++k) Dn[k] = Din[at + k];
  bool ok = true;
  pg::Chol6 c;
  if (i - s >= 0)
  {
    const long long lo = 36LL * (i - s);
    ok = pg::chol6(Din + lo, c) && ok;
    pg::chol6_right(c, Lin + at, X);
    for (int k = 0; k < 36; ++k) X[k] = -X[k];
    pg::mul6(X, Uin + lo, T);
    for (int k = 0; k < 36; ++k) Dn[k] += T[k];
    pg::mul6(X, Lin + lo, T);
    for (int k = 0; k < 36; ++k) { alpha[at + k] = X[k]; Lout[at + k] = T[k]; }
  }
  else
    for (int k = 0; k < 36; ++k) { alpha[at + k] = 0.; Lout[at + k] = 0.; }
  if (i + s < n)
  {
    const long long hi = 36LL * (i + s);
    ok = pg::chol6(Din + hi, c) && ok;
    pg::chol6_right(c, Uin + at, X);
    for (int k = 0; k < 36; ++k) X[k] = -X[k];
    pg::mul6(X, Lin + hi, T);
    for (int k = 0; k < 36; ++k) Dn[k] += T[k];
    pg::mul6(X, Uin + hi, T);
    for (int k = 0; k < 36; ++k) { gamma[at + k] = X[k]; Uout[at + k] = T[k]; }
  }
  else
    for (int k = 0; k < 36; ++k) { gamma[at + k] = 0.; Uout[at + k] = 0.; }
  for (int k = 0; k < 36; ++k) Dout[at + k] = Dn[k];
  if (!ok) st->notspd = 1;  // every writer writes the same word
}

// the inverses of the last level's diagonal blocks
__global__ __launch_bounds__(kThreads) void k_pgo_pcr_invert(int n, const double* __restrict__ D, double* __restrict__ Dinv, PgoState* st)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  pg::Chol6 c;
  const bool ok = pg::chol6(D + 36LL * i, c);
  for (int k = 0; k < 6; ++k)
  {
    double unit[6], col[6];
    for (int j = 0; j < 6; ++j) unit[j] = j == k ? 1. : 0.;
    pg::chol6_solve(c, unit, col);
    for (int j = 0; j < 6; ++j) Dinv[36LL * i + j * 6 + k] = col[j];
  }
  if (!ok) st->notspd = 1;
}

__global__ __launch_bounds__(kThreads) void k_pgo_pcr_apply(int n, int s, const double* __restrict__ alpha, const double* __restrict__ gamma, const double* __restrict__ bin,
                                                            double* __restrict__ bout)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double acc[6], y[6];
  for (int k = 0; k < 6; ++k) acc[k] = bin[6LL * i + k];
  if (i - s >= 0)
  {
    pg::mulv6(alpha + 36LL * i, bin + 6LL * (i - s), y);
    for (int k = 0; k < 6; ++k) acc[k] += y[k];
  }
  if (i + s < n)
  {
    pg::mulv6(gamma + 36LL * i, bin + 6LL * (i + s), y);
    for (int k = 0; k < 6; ++k) acc[k] += y[k];
  }
  for (int k = 0; k < 6; ++k) bout[6LL * i + k] = acc[k];
}

__global__ __launch_bounds__(kThreads) void k_pgo_pcr_solve(int n, const double* __restrict__ Dinv, const double* __restrict__ b, double* __restrict__ x)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double y[6];
  pg::mulv6(Dinv + 36LL * i, b + 6LL * i, y);
  for (int k = 0; k < 6; ++k) x[6LL * i + k] = y[k];
}

// the workgroup's sum by a fixed tree; every thread of the workgroup must call it
__device__ double block_sum(double v, double* lds)
{
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off) lds[threadIdx.x] = lds[threadIdx.x] + lds[threadIdx.x + off];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}
__device__ double block_max(double v, double* lds)
{
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1)
  {
    if ((int)threadIdx.x < off) lds[threadIdx.x] = lds[threadIdx.x + off] > lds[threadIdx.x] ? lds[threadIdx.x + off] : lds[threadIdx.x];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kThreads) void k_pgo_spmv(int n, pg::Graph G, const double* __restrict__ blocks, const double* __restrict__ D, const double* __restrict__ L,
                                                       const double* __restrict__ U, const double* __restrict__ p, double* __restrict__ q, double* __restrict__ partials)
{
  __shared__ double lds[kThreads];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  double d = 0.;
  if (i < n)
  {
    double y[6];
    pg::spmv_row(i, n, G, blocks, D, L, U, p, y);
    for (int k = 0; k < 6; ++k) q[6LL * i + k] = y[k];
    d = pg::dot6(p + 6LL * i, y);
  }
  const double s = block_sum(d, lds);
  if (threadIdx.x == 0 && partials) partials[blockIdx.x] = s;
}

// partial sums of a.b over the rows of six
__global__ __launch_bounds__(kThreads) void k_pgo_dot(int n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ partials)
{
  __shared__ double lds[kThreads];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const double s = block_sum(i < n ? pg::dot6(a + 6LL * i, b + 6LL * i) : 0., lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// partial sums of v[0..m)
__global__ __launch_bounds__(kThreads) void k_pgo_sum(int m, const double* __restrict__ v, double* __restrict__ partials)
{
  __shared__ double lds[kThreads];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const double s = block_sum(i < m ? v[i] : 0., lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}
// per workgroup: the model decrease's terms, max |delta|, max |g| (delta may be NULL: the gradient alone)
__global__ __launch_bounds__(kThreads) void k_pgo_row_stats(int n, double lambda, const double* __restrict__ delta, const double* __restrict__ dg, const double* __restrict__ g,
                                                            double* __restrict__ partials)
{
  __shared__ double lds[kThreads];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  double model = 0., md = 0., mg = 0.;
  if (i < n)
    for (int k = 0; k < 6; ++k)
    {
      const double gk = g[6LL * i + k];
      mg = __builtin_fabs(gk) > mg ? __builtin_fabs(gk) : mg;
      if (delta)
      {
        const double dk = delta[6LL * i + k];
        md = __builtin_fabs(dk) > md ? __builtin_fabs(dk) : md;
        const double t = dk * (lambda * dg[6LL * i + k] * dk - gk);
        model = k == 0 ? t : model + t;
      }
    }
  const double a = block_sum(model, lds), b = block_max(md, lds), c = block_max(mg, lds);
  if (threadIdx.x == 0)
  {
    partials[3LL * blockIdx.x] = a;
    partials[3LL * blockIdx.x + 1] = b;
    partials[3LL * blockIdx.x + 2] = c;
  }
}

// the second level: one thread adds the partial sums in order and takes PCG's decisions
enum { FIN_INIT = 0, FIN_PQ = 1, FIN_RZ = 2, FIN_STATS = 3, FIN_CHI2 = 4 };
__global__ void k_pgo_finish(int what, int nb, const double* __restrict__ partials, double tol2, PgoState* st)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (what == FIN_STATS)
  {
    double model = 0., md = 0., mg = 0.;
    for (int b = 0; b < nb; ++b)
    {
      model += partials[3LL * b];
      md = partials[3LL * b + 1] > md ? partials[3LL * b + 1] : md;
      mg = partials[3LL * b + 2] > mg ? partials[3LL * b + 2] : mg;
    }
    st->stat[0] = 0.5 * model;
    st->stat[1] = md;
    st->stat[2] = mg;
    return;
  }
  double s = 0.;
  for (int b = 0; b < nb; ++b) s += partials[b];
  if (what == FIN_CHI2) { st->stat[3] = s; return; }
  if (what == FIN_INIT)
  {
    st->rz = s;
    st->rz0 = s;
    st->iters = 0;
    st->converged = s == 0. ? 1 : 0;
    st->failed = (pg::finite_d(s) && s >= 0.) ? 0 : 1;
    return;
  }
  if (st->failed || st->converged) return;
  if (what == FIN_PQ)
  {
    st->pq = s;
    st->iters = st->iters + 1;
    if (!(s > 0.) || !pg::finite_d(s)) { st->failed = 1; st->alpha = 0.; }
    else st->alpha = st->rz / s;
    return;
  }
  // FIN_RZ
  if (!pg::finite_d(s)) { st->failed = 1; st->beta = 0.; return; }
  if (s <= tol2 * st->rz0) { st->converged = 1; st->beta = 0.; return; }
  st->beta = s / st->rz;
  st->rz = s;
}

__global__ __launch_bounds__(kThreads) void k_pgo_pcg_start(long long nv, const double* __restrict__ g, double* __restrict__ delta, double* __restrict__ r)
{
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= nv) return;
  delta[k] = 0.;
  r[k] = -g[k];
}
__global__ __launch_bounds__(kThreads) void k_pgo_axpy(long long nv, const PgoState* __restrict__ st, const double* __restrict__ p, const double* __restrict__ q,
                                                       double* __restrict__ delta, double* __restrict__ r)
{
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= nv || st->failed || st->converged) return;
  const double a = st->alpha;
  delta[k] += a * p[k];
  r[k] -= a * q[k];
}
__global__ __launch_bounds__(kThreads) void k_pgo_update_p(long long nv, const PgoState* __restrict__ st, const double* __restrict__ z, double* __restrict__ p)
{
  const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= nv || st->failed || st->converged) return;
  p[k] = z[k] + st->beta * p[k];
}
__global__ __launch_bounds__(kThreads) void k_pgo_retract(int n, const double* __restrict__ poses, const double* __restrict__ delta, double* __restrict__ cand)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  pg::store(pg::retract(pg::load(poses + 16LL * i), delta + 6LL * i), cand + 16LL * i);
}

// out_i = W P_i
__global__ __launch_bounds__(kThreads) void k_pgo_premultiply(int n, pg::Pose W, const double* __restrict__ poses, double* __restrict__ out)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  pg::store(pg::compose(W, pg::load(poses + 16LL * i)), out + 16LL * i);
}
// out_i = inv(P_0) P_i (out is another buffer than poses: every thread reads pose 0)
__global__ __launch_bounds__(kThreads) void k_pgo_reanchor(int n, const double* __restrict__ poses, double* __restrict__ out)
{
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  pg::store(pg::inverse_compose(pg::load(poses), pg::load(poses + 16LL * i)), out + 16LL * i);
}

int ensure(lsa_ctx* ctx, PgoBuf& b, size_t bytes)
{
  if (bytes <= b.cap) return LSA_OK;
  retire_dev(ctx, b.p);
  b.p = nullptr;
  b.cap = 0;
  const size_t cap = bytes + bytes / 2;
  LSA_HIP(ctx, hipMalloc(&b.p, cap));
  b.cap = cap;
  return LSA_OK;
}
template <typename T> T* ptr_of(const PgoBuf& b) { return static_cast<T*>(b.p); }

int levels_of(int n)
{
  int nl = 0;
  for (long long s = 1; s < n; s *= 2) ++nl;
  return nl;
}

// the vectors of PCG, 6 n doubles each
enum { V_DELTA = 0, V_R, V_Z, V_P, V_Q, V_T0, V_T1, V_COUNT };

struct Problem
{
  lsa_ctx* ctx;
  PgoBuffers* B;
  int n = 0, m = 0, k = 0, nl = 0, nb = 0;
  bool haveGraph = false;
  pg::Graph G{};
  pg::Pose O{};  // the priors' offset
  bool robust = false;  // a loss is set: the _robust kernels, the cost summed from B->cost
  PgoLoss loss{LSA_PGO_LOSS_NONE, LSA_PGO_LOSS_NONE, 1., 1., nullptr};
  double* vec(int k) const { return ptr_of<double>(B->vec) + 6LL * n * k; }
  PgoState* state() const { return ptr_of<PgoState>(B->state); }
};

#define PGO_TRY(call)                \
  do                                 \
  {                                  \
    const int rc__ = (call);         \
    if (rc__ != LSA_OK) return rc__; \
  } while (0)

// buffers for n poses, m edges and k priors; poses, edges, priors (and the graph, when given) uploaded
int setup(Problem& P, lsa_ctx* ctx, const double* poses16, int n, const unsigned char* fixed, const lsa_pgo_edge_t* edges, int m, const host::PoseGraph* G,
          const lsa_pgo_prior_t* priors = nullptr, int k = 0, const double* offset16 = nullptr, const unsigned char* mask = nullptr, const lsa_pgo_robust_t* rb = nullptr)
{
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->pgo) ctx->pgo = new PgoBuffers;
  PgoBuffers* B = ctx->pgo;
  P.ctx = ctx;
  P.B = B;
  P.n = n;
  P.m = m;
  P.k = k;
  if (k > 0) P.O = pg::load(offset16);
  P.nl = levels_of(n);
  P.nb = (int)blocks_for(std::max((long long)n, (long long)m + k));
  const size_t n36 = (size_t)n * 36 * sizeof(double), n6 = (size_t)n * 6 * sizeof(double);
  PGO_TRY(ensure(ctx, B->poses, (size_t)n * 16 * sizeof(double)));
  PGO_TRY(ensure(ctx, B->cand, (size_t)n * 16 * sizeof(double)));
  PGO_TRY(ensure(ctx, B->edges, std::max<size_t>(1, (size_t)m) * sizeof(lsa_pgo_edge_t)));
  PGO_TRY(ensure(ctx, B->fixed, (size_t)n));
  PGO_TRY(ensure(ctx, B->row_start, ((size_t)n + 1) * sizeof(int)));
  PGO_TRY(ensure(ctx, B->loop_start, ((size_t)n + 1) * sizeof(int)));
  PGO_TRY(ensure(ctx, B->inc, std::max<size_t>(1, (size_t)2 * m) * sizeof(int)));
  PGO_TRY(ensure(ctx, B->loop_edge, std::max<size_t>(1, (size_t)2 * m) * sizeof(int)));
  PGO_TRY(ensure(ctx, B->loop_col, std::max<size_t>(1, (size_t)2 * m) * sizeof(int)));
  PGO_TRY(ensure(ctx, B->e, std::max<size_t>(1, (size_t)m) * 6 * sizeof(double)));
  PGO_TRY(ensure(ctx, B->blocks, std::max<size_t>(1, (size_t)m) * pg::kEdgeBlock * sizeof(double)));
  PGO_TRY(ensure(ctx, B->chi2, std::max<size_t>(1, (size_t)m + (size_t)k) * sizeof(double)));
  PGO_TRY(ensure(ctx, B->priors, std::max<size_t>(1, (size_t)k) * sizeof(lsa_pgo_prior_t)));
  PGO_TRY(ensure(ctx, B->prior_start, ((size_t)n + 1) * sizeof(int)));
  PGO_TRY(ensure(ctx, B->prior_of, std::max<size_t>(1, (size_t)k) * sizeof(int)));
  PGO_TRY(ensure(ctx, B->pe, std::max<size_t>(1, (size_t)k) * 3 * sizeof(double)));
  PGO_TRY(ensure(ctx, B->pblocks, std::max<size_t>(1, (size_t)k) * pg::kPriorBlock * sizeof(double)));
  PGO_TRY(ensure(ctx, B->D, n36));
  PGO_TRY(ensure(ctx, B->L, n36));
  PGO_TRY(ensure(ctx, B->U, n36));
  PGO_TRY(ensure(ctx, B->dg, n6));
  PGO_TRY(ensure(ctx, B->g, n6));
  PGO_TRY(ensure(ctx, B->work[0], 3 * n36));
  PGO_TRY(ensure(ctx, B->work[1], 3 * n36));
  PGO_TRY(ensure(ctx, B->alpha, std::max(1, P.nl) * n36));
  PGO_TRY(ensure(ctx, B->gamma, std::max(1, P.nl) * n36));
  PGO_TRY(ensure(ctx, B->Dinv, n36));
  PGO_TRY(ensure(ctx, B->vec, V_COUNT * n6));
  PGO_TRY(ensure(ctx, B->partials, (size_t)3 * P.nb * sizeof(double)));
  PGO_TRY(ensure(ctx, B->state, sizeof(PgoState)));
  if (!B->host) LSA_HIP(ctx, hipHostMalloc((void**)&B->host, sizeof(PgoState), hipHostMallocDefault));
  hipStream_t st = ctx->stream;
  LSA_HIP(ctx, hipMemsetAsync(B->state.p, 0, sizeof(PgoState), st));
  if (poses16) LSA_HIP(ctx, hipMemcpyAsync(B->poses.p, poses16, (size_t)n * 16 * sizeof(double), hipMemcpyHostToDevice, st));
  if (m > 0 && edges) LSA_HIP(ctx, hipMemcpyAsync(B->edges.p, edges, (size_t)m * sizeof(lsa_pgo_edge_t), hipMemcpyHostToDevice, st));
  if (fixed) LSA_HIP(ctx, hipMemcpyAsync(B->fixed.p, fixed, (size_t)n, hipMemcpyHostToDevice, st));
  if (k > 0 && priors) LSA_HIP(ctx, hipMemcpyAsync(B->priors.p, priors, (size_t)k * sizeof(lsa_pgo_prior_t), hipMemcpyHostToDevice, st));
  if (rb && (rb->edge_loss != LSA_PGO_LOSS_NONE || rb->prior_loss != LSA_PGO_LOSS_NONE))
  {
    // the losses' own buffers; the mask travels once, with the edges
    P.robust = true;
    P.loss = PgoLoss{rb->edge_loss, rb->prior_loss, rb->edge_scale, rb->prior_scale, nullptr};
    PGO_TRY(ensure(ctx, B->cost, std::max<size_t>(1, (size_t)m + (size_t)k) * sizeof(double)));
    PGO_TRY(ensure(ctx, B->weight, std::max<size_t>(1, (size_t)m + (size_t)k) * sizeof(double)));
    if (mask && m > 0)
    {
      PGO_TRY(ensure(ctx, B->mask, (size_t)m));
      LSA_HIP(ctx, hipMemcpyAsync(B->mask.p, mask, (size_t)m, hipMemcpyHostToDevice, st));
      P.loss.mask = ptr_of<unsigned char>(B->mask);
    }
  }
  P.haveGraph = G != nullptr;
  if (G)
  {
    LSA_HIP(ctx, hipMemcpyAsync(B->row_start.p, G->row_start.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    LSA_HIP(ctx, hipMemcpyAsync(B->loop_start.p, G->loop_start.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (!G->inc.empty()) LSA_HIP(ctx, hipMemcpyAsync(B->inc.p, G->inc.data(), G->inc.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (!G->loop_edge.empty())
    {
      LSA_HIP(ctx, hipMemcpyAsync(B->loop_edge.p, G->loop_edge.data(), G->loop_edge.size() * sizeof(int), hipMemcpyHostToDevice, st));
      LSA_HIP(ctx, hipMemcpyAsync(B->loop_col.p, G->loop_col.data(), G->loop_col.size() * sizeof(int), hipMemcpyHostToDevice, st));
    }
    LSA_HIP(ctx, hipMemcpyAsync(B->prior_start.p, G->prior_start.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (!G->prior_of.empty()) LSA_HIP(ctx, hipMemcpyAsync(B->prior_of.p, G->prior_of.data(), G->prior_of.size() * sizeof(int), hipMemcpyHostToDevice, st));
    P.G = pg::Graph{ptr_of<int>(B->row_start), ptr_of<int>(B->inc), ptr_of<int>(B->loop_start), ptr_of<int>(B->loop_edge), ptr_of<int>(B->loop_col),
                    ptr_of<int>(B->prior_start), ptr_of<int>(B->prior_of)};
  }
  return LSA_OK;
}

int launch_linearize_priors(const Problem& P, const double* poses)
{
  if (P.k == 0) return LSA_OK;
  ProfScope ps(P.ctx, "pgo_linearize_priors", (double)P.k * (sizeof(lsa_pgo_prior_t) + (pg::kPriorBlock + 4) * 8.));
  if (P.robust)
    hipLaunchKernelGGL(k_pgo_linearize_priors_robust, dim3(blocks_for(P.k)), dim3(kThreads), 0, P.ctx->stream, poses, ptr_of<lsa_pgo_prior_t>(P.B->priors), P.k, P.O, P.loss,
                       ptr_of<double>(P.B->pe), ptr_of<double>(P.B->pblocks), ptr_of<double>(P.B->chi2) + P.m, ptr_of<double>(P.B->cost) + P.m,
                       ptr_of<double>(P.B->weight) + P.m);
  else
    hipLaunchKernelGGL(k_pgo_linearize_priors, dim3(blocks_for(P.k)), dim3(kThreads), 0, P.ctx->stream, poses, ptr_of<lsa_pgo_prior_t>(P.B->priors), P.k, P.O,
                       ptr_of<double>(P.B->pe), ptr_of<double>(P.B->pblocks), ptr_of<double>(P.B->chi2) + P.m);
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
// edges and priors
int launch_linearize(const Problem& P, const double* poses)
{
  if (P.m > 0)
  {
    ProfScope ps(P.ctx, "pgo_linearize", (double)P.m * (sizeof(lsa_pgo_edge_t) + (pg::kEdgeBlock + 7) * 8.));
    if (P.robust)
      hipLaunchKernelGGL(k_pgo_linearize_robust, dim3(blocks_for(P.m)), dim3(kThreads), 0, P.ctx->stream, poses, ptr_of<lsa_pgo_edge_t>(P.B->edges), P.m, P.loss,
                         ptr_of<double>(P.B->e), ptr_of<double>(P.B->blocks), ptr_of<double>(P.B->chi2), ptr_of<double>(P.B->cost), ptr_of<double>(P.B->weight));
    else
      hipLaunchKernelGGL(k_pgo_linearize, dim3(blocks_for(P.m)), dim3(kThreads), 0, P.ctx->stream, poses, ptr_of<lsa_pgo_edge_t>(P.B->edges), P.m, ptr_of<double>(P.B->e),
                         ptr_of<double>(P.B->blocks), ptr_of<double>(P.B->chi2));
    LSA_HIP(P.ctx, hipGetLastError());
  }
  return launch_linearize_priors(P, poses);
}
// the cost values of a candidate: chi2, or rho under a loss
int launch_candidate(const Problem& P, const double* cand)
{
  hipStream_t st = P.ctx->stream;
  if (P.robust)
  {
    if (P.m > 0) hipLaunchKernelGGL(k_pgo_chi2_robust<false>, dim3(blocks_for(P.m)), dim3(kThreads), 0, st, cand, ptr_of<lsa_pgo_edge_t>(P.B->edges), P.m, P.loss, ptr_of<double>(P.B->cost));
    if (P.k > 0)
      hipLaunchKernelGGL(k_pgo_chi2_priors_robust<false>, dim3(blocks_for(P.k)), dim3(kThreads), 0, st, cand, ptr_of<lsa_pgo_prior_t>(P.B->priors), P.k, P.O, P.loss,
                         ptr_of<double>(P.B->cost) + P.m);
  }
  else
  {
    if (P.m > 0) hipLaunchKernelGGL(k_pgo_chi2, dim3(blocks_for(P.m)), dim3(kThreads), 0, st, cand, ptr_of<lsa_pgo_edge_t>(P.B->edges), P.m, ptr_of<double>(P.B->chi2));
    if (P.k > 0)
      hipLaunchKernelGGL(k_pgo_chi2_priors, dim3(blocks_for(P.k)), dim3(kThreads), 0, st, cand, ptr_of<lsa_pgo_prior_t>(P.B->priors), P.k, P.O, ptr_of<double>(P.B->chi2) + P.m);
  }
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
// the verdicts {chi2, w} of the m edges and then the k priors at `poses`: the chi2 kernels once more, into B->verdict
int launch_verdicts(const Problem& P, const double* poses)
{
  hipStream_t st = P.ctx->stream;
  PGO_TRY(ensure(P.ctx, P.B->verdict, std::max<size_t>(1, (size_t)P.m + (size_t)P.k) * 2 * sizeof(double)));
  double* out = ptr_of<double>(P.B->verdict);
  if (P.m > 0) hipLaunchKernelGGL(k_pgo_chi2_robust<true>, dim3(blocks_for(P.m)), dim3(kThreads), 0, st, poses, ptr_of<lsa_pgo_edge_t>(P.B->edges), P.m, P.loss, out);
  if (P.k > 0)
    hipLaunchKernelGGL(k_pgo_chi2_priors_robust<true>, dim3(blocks_for(P.k)), dim3(kThreads), 0, st, poses, ptr_of<lsa_pgo_prior_t>(P.B->priors), P.k, P.O, P.loss, out + 2LL * P.m);
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
// sum of the cost values (the m edge values, then the k prior values: chi2, or rho under a loss) into stat[3]
int launch_cost(const Problem& P)
{
  const int nb = (int)blocks_for((long long)P.m + P.k);
  hipLaunchKernelGGL(k_pgo_sum, dim3(nb), dim3(kThreads), 0, P.ctx->stream, P.m + P.k, ptr_of<double>(P.robust ? P.B->cost : P.B->chi2), ptr_of<double>(P.B->partials));
  hipLaunchKernelGGL(k_pgo_finish, dim3(1), dim3(64), 0, P.ctx->stream, (int)FIN_CHI2, nb, ptr_of<double>(P.B->partials), 0., P.state());
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
int launch_assemble(const Problem& P, double lambda)
{
  ProfScope ps(P.ctx, "pgo_assemble", (double)P.n * (36 * 3 + 12) * 8. + (double)P.m * 2 * pg::kEdgeBlock * 8.);
  hipLaunchKernelGGL(k_pgo_assemble, dim3(blocks_for(P.n)), dim3(kThreads), 0, P.ctx->stream, P.n, ptr_of<unsigned char>(P.B->fixed), P.G, ptr_of<lsa_pgo_edge_t>(P.B->edges),
                     ptr_of<double>(P.B->blocks), ptr_of<double>(P.B->pblocks), lambda, ptr_of<double>(P.B->D), ptr_of<double>(P.B->dg), ptr_of<double>(P.B->g), ptr_of<double>(P.B->L),
                     ptr_of<double>(P.B->U));
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
// the cyclic reduction of (D, L, U): alpha / gamma per level and the last level's inverses; diagonalOnly: T = the D blocks
int launch_factor(const Problem& P, bool diagonalOnly)
{
  const int n = P.n;
  const long long n36 = 36LL * n;
  ProfScope ps(P.ctx, "pgo_factor", (double)(diagonalOnly ? 0 : P.nl) * n36 * 8. * 8 + n36 * 16.);
  const double* D = ptr_of<double>(P.B->D);
  const double* L = ptr_of<double>(P.B->L);
  const double* U = ptr_of<double>(P.B->U);
  int level = 0;
  if (!diagonalOnly)
    for (long long s = 1; s < n; s *= 2, ++level)
    {
      double* out = ptr_of<double>(P.B->work[level & 1]);
      hipLaunchKernelGGL(k_pgo_pcr_level, dim3(blocks_for(n)), dim3(kThreads), 0, P.ctx->stream, n, (int)s, D, L, U, out, out + n36, out + 2 * n36,
                         ptr_of<double>(P.B->alpha) + level * n36, ptr_of<double>(P.B->gamma) + level * n36, P.state());
      D = out;
      L = out + n36;
      U = out + 2 * n36;
    }
  hipLaunchKernelGGL(k_pgo_pcr_invert, dim3(blocks_for(n)), dim3(kThreads), 0, P.ctx->stream, n, D, ptr_of<double>(P.B->Dinv), P.state());
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
// x = T^-1 b (b is kept)
int launch_apply(const Problem& P, bool diagonalOnly, const double* b, double* x)
{
  const int n = P.n;
  const long long n36 = 36LL * n;
  ProfScope ps(P.ctx, "pgo_apply", (double)((diagonalOnly ? 0 : P.nl) * 2 + 1) * (n36 + 12LL * n) * 8.);
  const double* in = b;
  int level = 0;
  if (!diagonalOnly)
    for (long long s = 1; s < n; s *= 2, ++level)
    {
      double* out = P.vec(V_T0 + (level & 1));
      hipLaunchKernelGGL(k_pgo_pcr_apply, dim3(blocks_for(n)), dim3(kThreads), 0, P.ctx->stream, n, (int)s, ptr_of<double>(P.B->alpha) + level * n36,
                         ptr_of<double>(P.B->gamma) + level * n36, in, out);
      in = out;
    }
  hipLaunchKernelGGL(k_pgo_pcr_solve, dim3(blocks_for(n)), dim3(kThreads), 0, P.ctx->stream, n, ptr_of<double>(P.B->Dinv), in, x);
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
int launch_spmv(const Problem& P, const double* p, double* q, double* partials)
{
  ProfScope ps(P.ctx, "pgo_spmv", (double)P.n * (36 * 3 + 12) * 8.);
  hipLaunchKernelGGL(k_pgo_spmv, dim3(blocks_for(P.n)), dim3(kThreads), 0, P.ctx->stream, P.n, P.G, ptr_of<double>(P.B->blocks), ptr_of<double>(P.B->D),
                     ptr_of<double>(P.B->L), ptr_of<double>(P.B->U), p, q, partials);
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
int finish(const Problem& P, int what, int nb, double tol2)
{
  hipLaunchKernelGGL(k_pgo_finish, dim3(1), dim3(64), 0, P.ctx->stream, what, nb, ptr_of<double>(P.B->partials), tol2, P.state());
  LSA_HIP(P.ctx, hipGetLastError());
  return LSA_OK;
}
int read_state(const Problem& P, PgoState* out)
{
  LSA_HIP(P.ctx, hipMemcpyAsync(P.B->host, P.B->state.p, sizeof(PgoState), hipMemcpyDeviceToHost, P.ctx->stream));
  LSA_HIP(P.ctx, hipStreamSynchronize(P.ctx->stream));
  *out = *P.B->host;
  return LSA_OK;
}
int download(lsa_ctx* ctx, void* dst, const void* src, size_t bytes)
{
  if (bytes) LSA_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return LSA_OK;
}
}  // namespace

extern "C" {

int lsa_pgo_linearize(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, double* e_out, double* blocks_out, double* chi2_out)
{
  if (!ctx) return LSA_E_ARG;
  std::string why = "bad argument";
  if (!e_out || !blocks_out || !chi2_out || host::PgoCheckEdges(poses16, n, edges, m, &why) != LSA_OK) return ctx->fail(LSA_E_ARG, "lsa_pgo_linearize: " + why);
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_linearize: more than 262144 poses");
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, nullptr, edges, m, nullptr));
  PGO_TRY(launch_linearize(P, ptr_of<double>(P.B->poses)));
  PGO_TRY(download(ctx, e_out, P.B->e.p, (size_t)m * 6 * sizeof(double)));
  PGO_TRY(download(ctx, blocks_out, P.B->blocks.p, (size_t)m * pg::kEdgeBlock * sizeof(double)));
  PGO_TRY(download(ctx, chi2_out, P.B->chi2.p, (size_t)m * sizeof(double)));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

int lsa_pgo_assemble(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, double* D_out, double* g_out,
                     double* L_out, double* U_out)
{
  return lsa_pgo_assemble_priors(ctx, poses16, n, fixed, edges, m, nullptr, 0, nullptr, lambda, D_out, g_out, L_out, U_out);
}

int lsa_pgo_assemble_priors(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                            const double* offset16, double lambda, double* D_out, double* g_out, double* L_out, double* U_out)
{
  if (!ctx) return LSA_E_ARG;
  std::string why = "bad argument";
  host::PoseGraph G;
  if (!D_out || !g_out || !L_out || !U_out || !(lambda >= 0.) || !pg::finite_d(lambda) ||
      host::PgoBuild(poses16, n, fixed, edges, m, &G, &why, priors, k, offset16) != LSA_OK)
    return ctx->fail(LSA_E_ARG, "lsa_pgo_assemble: " + why);
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_assemble: more than 262144 poses");
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, fixed, edges, m, &G, priors, k, offset16));
  PGO_TRY(launch_linearize(P, ptr_of<double>(P.B->poses)));
  PGO_TRY(launch_assemble(P, lambda));
  const size_t n36 = (size_t)n * 36 * sizeof(double);
  PGO_TRY(download(ctx, D_out, P.B->D.p, n36));
  PGO_TRY(download(ctx, g_out, P.B->g.p, (size_t)n * 6 * sizeof(double)));
  PGO_TRY(download(ctx, L_out, P.B->L.p, n36));
  PGO_TRY(download(ctx, U_out, P.B->U.p, n36));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

int lsa_pgo_spmv(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, const double* p, double* q)
{
  return lsa_pgo_spmv_priors(ctx, poses16, n, fixed, edges, m, nullptr, 0, nullptr, lambda, p, q);
}

int lsa_pgo_spmv_priors(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                        const double* offset16, double lambda, const double* p, double* q)
{
  if (!ctx) return LSA_E_ARG;
  std::string why = "bad argument";
  host::PoseGraph G;
  if (!p || !q || !(lambda >= 0.) || !pg::finite_d(lambda) || host::PgoBuild(poses16, n, fixed, edges, m, &G, &why, priors, k, offset16) != LSA_OK)
    return ctx->fail(LSA_E_ARG, "lsa_pgo_spmv: " + why);
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_spmv: more than 262144 poses");
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, fixed, edges, m, &G, priors, k, offset16));
  PGO_TRY(launch_linearize(P, ptr_of<double>(P.B->poses)));
  PGO_TRY(launch_assemble(P, lambda));
  LSA_HIP(ctx, hipMemcpyAsync(P.vec(V_P), p, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PGO_TRY(launch_spmv(P, P.vec(V_P), P.vec(V_Q), nullptr));
  PGO_TRY(download(ctx, q, P.vec(V_Q), (size_t)n * 6 * sizeof(double)));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

int lsa_pgo_retract(lsa_ctx* ctx, const double* poses16, int n, const double* delta, double* poses_out)
{
  if (!ctx) return LSA_E_ARG;
  if (!poses16 || !delta || !poses_out || n < 1) return ctx->fail(LSA_E_ARG, "lsa_pgo_retract: bad argument");
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_retract: more than 262144 poses");
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, nullptr, nullptr, 0, nullptr));
  LSA_HIP(ctx, hipMemcpyAsync(P.vec(V_DELTA), delta, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_pgo_retract, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, ptr_of<double>(P.B->poses), P.vec(V_DELTA), ptr_of<double>(P.B->cand));
  LSA_HIP(ctx, hipGetLastError());
  std::vector<double> out((size_t)n * 16);
  PGO_TRY(download(ctx, out.data(), P.B->cand.p, out.size() * sizeof(double)));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(poses_out, out.data(), out.size() * sizeof(double));
  return LSA_OK;
}

int lsa_pgo_tridiagonal_solve(lsa_ctx* ctx, int n, const double* D, const double* L, const double* U, const double* b, double* x)
{
  if (!ctx) return LSA_E_ARG;
  if (n < 1 || !D || !L || !U || !b || !x) return ctx->fail(LSA_E_ARG, "lsa_pgo_tridiagonal_solve: bad argument");
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_tridiagonal_solve: more than 262144 rows");
  Problem P;
  PGO_TRY(setup(P, ctx, nullptr, n, nullptr, nullptr, 0, nullptr));
  const size_t n36 = (size_t)n * 36 * sizeof(double);
  hipStream_t st = ctx->stream;
  LSA_HIP(ctx, hipMemcpyAsync(P.B->D.p, D, n36, hipMemcpyHostToDevice, st));
  LSA_HIP(ctx, hipMemcpyAsync(P.B->L.p, L, n36, hipMemcpyHostToDevice, st));
  LSA_HIP(ctx, hipMemcpyAsync(P.B->U.p, U, n36, hipMemcpyHostToDevice, st));
  LSA_HIP(ctx, hipMemcpyAsync(P.vec(V_R), b, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, st));
  PGO_TRY(launch_factor(P, false));
  PGO_TRY(launch_apply(P, false, P.vec(V_R), P.vec(V_Z)));
  PgoState s;
  PGO_TRY(read_state(P, &s));
  if (s.notspd) return 1;
  std::vector<double> out((size_t)n * 6);
  PGO_TRY(download(ctx, out.data(), P.vec(V_Z), out.size() * sizeof(double)));
  LSA_HIP(ctx, hipStreamSynchronize(st));
  for (double v : out)
    if (!pg::finite_d(v)) return 1;
  std::memcpy(x, out.data(), out.size() * sizeof(double));
  return LSA_OK;
}

int lsa_pgo_solve(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_params_t* params, double* poses_out,
                  lsa_pgo_result_t* result)
{
  return lsa_pgo_solve_priors(ctx, poses16, n, fixed, edges, m, nullptr, 0, nullptr, params, poses_out, result);
}

int lsa_pgo_linearize_priors(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, double* e_out, double* blocks_out,
                             double* chi2_out)
{
  if (!ctx) return LSA_E_ARG;
  std::string why = "bad argument";
  if (!e_out || !blocks_out || !chi2_out || host::PgoCheckPriors(poses16, n, priors, k, offset16, &why) != LSA_OK)
    return ctx->fail(LSA_E_ARG, "lsa_pgo_linearize_priors: " + why);
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_linearize_priors: more than 262144 poses");
  if (k == 0) return LSA_OK;
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, nullptr, nullptr, 0, nullptr, priors, k, offset16));
  PGO_TRY(launch_linearize_priors(P, ptr_of<double>(P.B->poses)));
  PGO_TRY(download(ctx, e_out, P.B->pe.p, (size_t)k * 3 * sizeof(double)));
  PGO_TRY(download(ctx, blocks_out, P.B->pblocks.p, (size_t)k * pg::kPriorBlock * sizeof(double)));
  PGO_TRY(download(ctx, chi2_out, P.B->chi2.p, (size_t)k * sizeof(double)));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

// the two transforms around a solve with priors; what = 0: W P_i, 1: inv(P_0) P_i
static int pgo_transform(lsa_ctx* ctx, const char* who, int what, const double* poses16, int n, const double* W16, double* poses_out)
{
  if (!ctx) return LSA_E_ARG;
  if (!poses16 || !poses_out || n < 1 || (what == 0 && !W16)) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": more than 262144 poses");
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, nullptr, nullptr, 0, nullptr));
  if (what == 0)
    hipLaunchKernelGGL(k_pgo_premultiply, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, pg::load(W16), ptr_of<double>(P.B->poses), ptr_of<double>(P.B->cand));
  else
    hipLaunchKernelGGL(k_pgo_reanchor, dim3(blocks_for(n)), dim3(kThreads), 0, ctx->stream, n, ptr_of<double>(P.B->poses), ptr_of<double>(P.B->cand));
  LSA_HIP(ctx, hipGetLastError());
  std::vector<double> out((size_t)n * 16);
  PGO_TRY(download(ctx, out.data(), P.B->cand.p, out.size() * sizeof(double)));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(poses_out, out.data(), out.size() * sizeof(double));
  return LSA_OK;
}
int lsa_pgo_premultiply(lsa_ctx* ctx, const double* poses16, int n, const double* W16, double* poses_out)
{
  return pgo_transform(ctx, "lsa_pgo_premultiply", 0, poses16, n, W16, poses_out);
}
int lsa_pgo_reanchor(lsa_ctx* ctx, const double* poses16, int n, double* poses_out) { return pgo_transform(ctx, "lsa_pgo_reanchor", 1, poses16, n, nullptr, poses_out); }

int lsa_pgo_solve_priors(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                         const double* offset16, const lsa_pgo_params_t* params, double* poses_out, lsa_pgo_result_t* result)
{
  return lsa_pgo_solve_robust(ctx, poses16, n, fixed, edges, m, nullptr, priors, k, offset16, params, nullptr, poses_out, result, nullptr, nullptr);
}

int lsa_pgo_solve_robust(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask,
                         const lsa_pgo_prior_t* priors, int k, const double* offset16, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust, double* poses_out,
                         lsa_pgo_result_t* result, double* edge_verdict_out, double* prior_verdict_out)
{
  if (!ctx) return LSA_E_ARG;
  lsa_pgo_params_t p;
  lsa_pgo_params_init(&p);
  if (params) p = *params;
  lsa_pgo_robust_t rb;
  lsa_pgo_robust_init(&rb);
  if (robust) rb = *robust;
  if (!poses_out || !result || !pg::params_ok(p)) return ctx->fail(LSA_E_ARG, "lsa_pgo_solve: bad argument or parameters out of limits");
  if (!pg::robust_ok(rb)) return ctx->fail(LSA_E_ARG, "lsa_pgo_solve: a loss outside 0..3, or a scale that is not finite and positive");
  std::string why;
  host::PoseGraph G;
  if (const int rc = host::PgoBuild(poses16, n, fixed, edges, m, &G, &why, priors, k, offset16); rc != LSA_OK) return ctx->fail(rc, "lsa_pgo_solve: " + why);
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_solve: more than 262144 poses (the cyclic reduction keeps every level)");
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, fixed, edges, m, &G, priors, k, offset16, edge_mask, &rb));
  hipStream_t st = ctx->stream;
  const long long nv = 6LL * n;
  const bool diag = p.preconditioner == 1;
  double* x = ptr_of<double>(P.B->poses);
  double* cand = ptr_of<double>(P.B->cand);
  double* partials = ptr_of<double>(P.B->partials);
  const int nbn = (int)blocks_for(n);
  PgoState s;
  lsa_pgo_result_t R;
  std::memset(&R, 0, sizeof(R));
  PGO_TRY(launch_linearize(P, x));
  PGO_TRY(launch_cost(P));
  PGO_TRY(read_state(P, &s));
  double F = 0.5 * s.stat[3];
  R.initial_cost = F;
  double lambda = p.initial_lambda;
  int term = LSA_PGO_MAX_ITERATIONS;
  for (int it = 0; it < p.max_iterations; ++it)
  {
    R.iterations = it + 1;
    LSA_HIP(ctx, hipMemsetAsync(P.B->state.p, 0, sizeof(PgoState), st));
    PGO_TRY(launch_assemble(P, lambda));
    hipLaunchKernelGGL(k_pgo_row_stats, dim3(nbn), dim3(kThreads), 0, st, n, lambda, (const double*)nullptr, ptr_of<double>(P.B->dg), ptr_of<double>(P.B->g), partials);
    PGO_TRY(finish(P, FIN_STATS, nbn, 0.));
    // the factorization and PCG's start are enqueued behind the gradient's norm: one wait for all of them
    PGO_TRY(launch_factor(P, diag));
    hipLaunchKernelGGL(k_pgo_pcg_start, dim3(blocks_for(nv)), dim3(kThreads), 0, st, nv, ptr_of<double>(P.B->g), P.vec(V_DELTA), P.vec(V_R));
    PGO_TRY(launch_apply(P, diag, P.vec(V_R), P.vec(V_Z)));
    LSA_HIP(ctx, hipMemcpyAsync(P.vec(V_P), P.vec(V_Z), (size_t)nv * sizeof(double), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_pgo_dot, dim3(nbn), dim3(kThreads), 0, st, n, P.vec(V_R), P.vec(V_Z), partials);
    PGO_TRY(finish(P, FIN_INIT, nbn, 0.));
    PGO_TRY(read_state(P, &s));
    if (s.stat[2] <= p.gradient_tolerance) { term = LSA_PGO_GRADIENT; break; }
    if (s.notspd) { term = LSA_PGO_LINEAR_SOLVER_FAILED; break; }
    int iters = 0;
    while (!s.converged && !s.failed && iters < p.pcg_max_iter)
    {
      ++iters;
      PGO_TRY(launch_spmv(P, P.vec(V_P), P.vec(V_Q), partials));
      PGO_TRY(finish(P, FIN_PQ, nbn, 0.));
      hipLaunchKernelGGL(k_pgo_axpy, dim3(blocks_for(nv)), dim3(kThreads), 0, st, nv, P.state(), P.vec(V_P), P.vec(V_Q), P.vec(V_DELTA), P.vec(V_R));
      PGO_TRY(launch_apply(P, diag, P.vec(V_R), P.vec(V_Z)));
      hipLaunchKernelGGL(k_pgo_dot, dim3(nbn), dim3(kThreads), 0, st, n, P.vec(V_R), P.vec(V_Z), partials);
      PGO_TRY(finish(P, FIN_RZ, nbn, p.pcg_tolerance * p.pcg_tolerance));
      hipLaunchKernelGGL(k_pgo_update_p, dim3(blocks_for(nv)), dim3(kThreads), 0, st, nv, P.state(), P.vec(V_Z), P.vec(V_P));
      PGO_TRY(read_state(P, &s));
    }
    R.pcg_iterations += iters;
    R.last_pcg_iterations = iters;
    if (s.failed) { term = LSA_PGO_LINEAR_SOLVER_FAILED; break; }
    if (!s.converged) ++R.pcg_truncated;
    hipLaunchKernelGGL(k_pgo_row_stats, dim3(nbn), dim3(kThreads), 0, st, n, lambda, P.vec(V_DELTA), ptr_of<double>(P.B->dg), ptr_of<double>(P.B->g), partials);
    PGO_TRY(finish(P, FIN_STATS, nbn, 0.));
    hipLaunchKernelGGL(k_pgo_retract, dim3(nbn), dim3(kThreads), 0, st, n, x, P.vec(V_DELTA), cand);
    PGO_TRY(launch_candidate(P, cand));
    PGO_TRY(launch_cost(P));
    PGO_TRY(read_state(P, &s));
    const double model = s.stat[0], step = s.stat[1], Fn = 0.5 * s.stat[3];
    if (model > 0. && pg::finite_d(Fn) && F - Fn > 0.)
    {
      const double dec = F - Fn;
      std::swap(x, cand);
      const bool small = dec <= p.cost_tolerance * F;
      PGO_TRY(launch_linearize(P, x));
      PGO_TRY(launch_cost(P));
      PGO_TRY(read_state(P, &s));
      F = 0.5 * s.stat[3];
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
  R.message = host::PgoMessage(term);
  std::vector<double> out((size_t)n * 16), verdict;
  if (edge_verdict_out || prior_verdict_out)
  {
    verdict.resize(((size_t)m + (size_t)k) * 2);
    PGO_TRY(launch_verdicts(P, x));
    PGO_TRY(download(ctx, verdict.data(), P.B->verdict.p, verdict.size() * sizeof(double)));
  }
  PGO_TRY(download(ctx, out.data(), x, out.size() * sizeof(double)));
  LSA_HIP(ctx, hipStreamSynchronize(st));
  std::memcpy(poses_out, out.data(), out.size() * sizeof(double));
  if (edge_verdict_out && m > 0) std::memcpy(edge_verdict_out, verdict.data(), (size_t)m * 2 * sizeof(double));
  if (prior_verdict_out && k > 0) std::memcpy(prior_verdict_out, verdict.data() + (size_t)m * 2, (size_t)k * 2 * sizeof(double));
  *result = R;
  return LSA_OK;
}

int lsa_pgo_linearize_robust(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask, const lsa_pgo_robust_t* robust,
                             double* e_out, double* blocks_out, double* chi2_out, double* rho_out, double* w_out)
{
  if (!ctx) return LSA_E_ARG;
  std::string why = "bad argument";
  lsa_pgo_robust_t rb;
  lsa_pgo_robust_init(&rb);
  if (robust) rb = *robust;
  if (!e_out || !blocks_out || !chi2_out || !rho_out || !w_out || !pg::robust_ok(rb) || host::PgoCheckEdges(poses16, n, edges, m, &why) != LSA_OK)
    return ctx->fail(LSA_E_ARG, "lsa_pgo_linearize_robust: " + why);
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_linearize_robust: more than 262144 poses");
  if (m == 0) return LSA_OK;
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, nullptr, edges, m, nullptr, nullptr, 0, nullptr, edge_mask, &rb));
  PGO_TRY(launch_linearize(P, ptr_of<double>(P.B->poses)));
  PGO_TRY(download(ctx, e_out, P.B->e.p, (size_t)m * 6 * sizeof(double)));
  PGO_TRY(download(ctx, blocks_out, P.B->blocks.p, (size_t)m * pg::kEdgeBlock * sizeof(double)));
  PGO_TRY(download(ctx, chi2_out, P.B->chi2.p, (size_t)m * sizeof(double)));
  if (P.robust)
  {
    PGO_TRY(download(ctx, rho_out, P.B->cost.p, (size_t)m * sizeof(double)));
    PGO_TRY(download(ctx, w_out, P.B->weight.p, (size_t)m * sizeof(double)));
  }
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!P.robust)  // no loss: the plain kernel ran; rho = chi2, w = 1
    for (int a = 0; a < m; ++a) { rho_out[a] = chi2_out[a]; w_out[a] = 1.; }
  return LSA_OK;
}

int lsa_pgo_linearize_robust_priors(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, const lsa_pgo_robust_t* robust,
                                    double* e_out, double* blocks_out, double* chi2_out, double* rho_out, double* w_out)
{
  if (!ctx) return LSA_E_ARG;
  std::string why = "bad argument";
  lsa_pgo_robust_t rb;
  lsa_pgo_robust_init(&rb);
  if (robust) rb = *robust;
  if (!e_out || !blocks_out || !chi2_out || !rho_out || !w_out || !pg::robust_ok(rb) || host::PgoCheckPriors(poses16, n, priors, k, offset16, &why) != LSA_OK)
    return ctx->fail(LSA_E_ARG, "lsa_pgo_linearize_robust_priors: " + why);
  if (n > kMaxPoses) return ctx->fail(LSA_E_CAPACITY, "lsa_pgo_linearize_robust_priors: more than 262144 poses");
  if (k == 0) return LSA_OK;
  Problem P;
  PGO_TRY(setup(P, ctx, poses16, n, nullptr, nullptr, 0, nullptr, priors, k, offset16, nullptr, &rb));
  PGO_TRY(launch_linearize_priors(P, ptr_of<double>(P.B->poses)));
  PGO_TRY(download(ctx, e_out, P.B->pe.p, (size_t)k * 3 * sizeof(double)));
  PGO_TRY(download(ctx, blocks_out, P.B->pblocks.p, (size_t)k * pg::kPriorBlock * sizeof(double)));
  PGO_TRY(download(ctx, chi2_out, P.B->chi2.p, (size_t)k * sizeof(double)));
  if (P.robust)
  {
    PGO_TRY(download(ctx, rho_out, P.B->cost.p, (size_t)k * sizeof(double)));
    PGO_TRY(download(ctx, w_out, P.B->weight.p, (size_t)k * sizeof(double)));
  }
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (!P.robust)
    for (int a = 0; a < k; ++a) { rho_out[a] = chi2_out[a]; w_out[a] = 1.; }
  return LSA_OK;
}

}  // extern "C"
