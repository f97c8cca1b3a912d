// lsa_pose_graph.h -- the pose graph of relative-pose edges and position priors and its Levenberg-Marquardt solve, ONE definition for the host
// statement (host/lsa_pose_graph.cpp) and the device (lsa_pose_graph.hip); DESIGN.md 3.9.  Plain C++ in double precision (no
// HIP header, no libm): sines, cosines and atan2 are lsa_pmath.h's, sqrt and / the IEEE ones, nothing may be contracted or
// re-associated (-ffp-contract=off), so the same inputs give the same bits wherever this text is compiled.
//
// VERTEX  a rigid pose (R, t); a row-major 4x4 at the ABI.
// RETRACTION by delta = (rho, phi) in R^6:   t <- t + R rho,   R <- R Exp(phi).
// EDGE (i, j, Z = (Rz, tz), Omega 6x6) with d = Ri^T (tj - ti), Rij = Ri^T Rj, RE = Rz^T Rij:
//   e = [ Rz^T (d - tz) ; Log(RE) ]
//   A = de/ddelta_i = [ -Rz^T , Rz^T [d]x ; 0 , -J Rij^T ]      B = de/ddelta_j = [ RE , 0 ; 0 , J ]
//   J = Jr^-1(e_rot) = I + 1/2 [phi]x + c(theta) [phi]x^2,   c = 1/theta^2 - (1 + cos theta) / (2 theta sin theta).
// A rotation error of exactly pi is outside the definition (Log has no unique value there, c has a pole at 2 pi).
//
// PRIOR (i, g, Omega 3x3): a measured position g of a point carried by pose i (a GPS antenna).  All priors of a solve share one
//   offset O = (Ro, to), the inverse of the antenna's pose in the body (what the reference gives g2o's ParameterSE3Offset).
//   d = Ri^T (g - ti)      e = Ro^T (d - to)      A = de/ddelta_i = [ -Ro^T , Ro^T [d]x ]  (3x6)
//   (g2o's EdgeSE3PointXYZ with a zero measurement.  Omega weighs e in this antenna frame although a GPS covariance is given
//   in the world frame: the reference's letter, kept.)  With no fixed pose and fewer than three non-collinear priors the
//   minimum is not unique: outside the definition, as a rotation error of pi is.
//
// SMALL ANGLES AND ANGLES NEAR PI
//   Exp:  R = I + a [phi]x + b [phi]x^2.  theta^2 < 1e-8: a = 1 - theta^2/6, b = 1/2 - theta^2/24 (the next terms are below
//         1e-17); else a = sin(theta)/theta, b = 2 sin^2(theta/2)/theta^2 (no 1 - cos: nothing cancels).
//   Log:  the unit quaternion of R (Eigen's four branches), negated when w < 0, so w >= 0 and theta = 2 atan2(|v|, w) in
//         [0, pi]; phi = k v with k = theta/|v|, and k = (2/w)(1 - |v|^2/(3 w^2)) when |v|^2 < 1e-10.
//   c:    theta^2 < 1/16: the series 1/12 + t/720 + t^2/30240 + t^3/1209600 + t^4/47900160 + 691 t^5/1307674368000 in
//         t = theta^2 (the first term left out is below 2e-17); else (1 - h cos(h)/sin(h))/theta^2 with h = theta/2, which is the
//         formula above with (1 + cos)/sin written as cot(theta/2): accurate up to pi, where sin(theta) vanishes.
//
// ORDER OF THE SUMS.  A product of two 3x3 or 6x6 matrices, and of a matrix and a vector, sums over the inner index
// ascending, left to right, starting from the first product.  Per edge: OA = Omega A, OB = Omega B, Oe = Omega e; then
// Haa = A^T OA, Hab = A^T OB, Hbb = B^T OB, ga = A^T Oe, gb = B^T Oe, chi2 = e^T Oe -- the 120 doubles of an edge's block
// record in that order (kEdgeBlock), 6x6 row-major.  Per prior: OA = Omega A (3x6), Oe = Omega e; Haa = A^T OA, ga = A^T Oe,
// chi2 = e^T Oe -- the 42 doubles of a prior's block record (kPriorBlock).
// ASSEMBLY.  Diagonal block D_i and gradient g_i of a free pose i: the sums of Haa / ga (i = from) or Hbb / gb (i = to) over
// its incident edges in ascending edge index, starting from the first.  Off-diagonal block (i, j): the sum over the edges
// joining i and j in ascending edge index of Hab (i = from) or Hab^T (i = to).  The priors of pose i follow its edges in D_i and
// g_i, in ascending prior index (a second list, prior_start / prior_of); they touch no other block.  A fixed pose: delta = 0, its
// row is the identity, g = 0, couplings to it are dropped, a prior on it counts in the cost alone.  H_lambda = H + lambda diag(H): on the diagonal h + lambda * h.
// PRECONDITIONER  T = the blocks of H_lambda with |i - j| <= 1 (SPD whenever H_lambda is: chain edges enter whole, other edges by
// their diagonal blocks, the damping is positive); every other block is PCG's.
//
// THE LM LOOP (the host and the device follow this text; p = lsa_pgo_params_t)
//   x = poses; linearize; F = 1/2 sum rho_k (the edges' values in edge order, then the priors' in prior order; rho_k = chi2_k without a loss); F0 = F;
//   lambda = p.initial_lambda
//   for it = 0 .. p.max_iterations - 1:
//     assemble at lambda;  if max |g| <= p.gradient_tolerance: GRADIENT
//     factor T;  a block that is not SPD: LINEAR_SOLVER_FAILED (poses as they were before this iteration)
//     PCG on H_lambda delta = -g:  delta = 0, r = -g, z = T^-1 r, p = z, rz0 = rz = r.z;  unless rz0 == 0, k = 1 .. p.pcg_max_iter:
//         q = H_lambda p; pq = p.q; not (pq > 0) or not finite: LINEAR_SOLVER_FAILED;  alpha = rz / pq;  delta += alpha p;
//         r -= alpha q;  z = T^-1 r;  rz' = r.z;  rz' <= p.pcg_tolerance^2 rz0: done;  beta = rz' / rz;  p = z + beta p;  rz = rz'
//       running out of iterations is no failure: LM takes the delta it has (counted in pcg_truncated)
//     step = max |delta|;  model = 1/2 sum_k delta_k (lambda diag(H)_k delta_k - g_k);  candidate = retraction;  F' = its cost 1/2 sum rho_k
//     accept when model > 0, F' finite and F - F' > 0 (the gain ratio (F - F') / model is positive):
//         x = candidate; lambda = max(lambda * p.lambda_shrink, p.lambda_min); then step <= p.step_tolerance: STEP;
//         (F - F') <= p.cost_tolerance * F: COST (both tested after the step was taken)
//     else lambda *= p.lambda_grow;  step <= p.step_tolerance: STEP;  lambda > p.lambda_max: LAMBDA_CEILING
//   MAX_ITERATIONS
// Every loop is bounded by a parameter: LM by max_iterations, PCG by pcg_max_iter.
//
// ROBUST LOSS (lsa_pgo_robust_t).  A loss acts on s = chi2 of one constraint, the squared Mahalanobis norm above,
// with a scale c > 0 in sigmas, c2 = c * c.  It yields the cost value rho(s) and the weight w = rho'(s).  First-order IRLS: the
// weight alone, no second-derivative correction (g2o's rule).  No transcendental function: IEEE sqrt, *, /, + under
// -ffp-contract=off pin the bits.  The order of operations below is part of the definition.
//   NONE 0             rho = s                                                     w = 1; nothing is multiplied
//   HUBER 1            s > c2:  r = sqrt(s);  rho = (2 * c) * r - c2               w = c / r
//                      else     rho = s                                            w = 1
//   GEMAN_MCCLURE 2    d = c2 + s;  rho = (c2 * s) / d                             q = c2 / d;  w = q * q
//   TUKEY 3            s > c2:  rho = c2 / 3                                       w = 0
//                      else     v = 1 - s / c2;  rho = (s / 3) * ((1 + v) + v * v) w = v * v
// Tukey's inner form is c2/3 (1 - v^3) without the cancellation, so rho -> s for small s (Ceres' TukeyLoss, the loss the ICP
// solve uses).  The outer branch is taken only when s > c2 is TRUE: a NaN chi2 stays a NaN cost and the LM loop rejects it as it
// always did.  An indefinite information matrix that drives s <= -c2 under Geman-McClure is outside the definition.
// Which constraints: edge_mask[m] (bytes; NULL = every edge) selects the edges edge_loss / edge_scale act on; prior_loss /
// prior_scale act on every prior.  Linearization of a robustified constraint: e, the block record and chi2 exactly as above,
// then blk[t] = w * blk[t] for t ascending (120 doubles of an edge, 42 of a prior); the value that enters F is rho; e and the raw
// chi2 are kept.  A constraint that is not robustified -- an unmasked edge, or a loss NONE -- is left untouched.  Assembly,
// H_lambda, the preconditioner, PCG, the model decrease and the accept rule read the weighted records and are as above.
// Geman-McClure and Tukey are not convex: the loop finds the minimum nearest its start (the Slam calls start from the logged
// odometry, the usual choice).  After the loop one more evaluation at the returned poses gives every constraint's VERDICT
// {chi2, w}; w = 1 for a constraint that is not robustified.
#pragma once
#include "../../include/lidarslam_amd.h"
#include "../../include/lsa_pmath.h"

namespace lsa
{
namespace pg
{
constexpr int kEdgeBlock = 120;  // Haa[36] Hab[36] Hbb[36] ga[6] gb[6]
constexpr int kPriorBlock = 42;  // Haa[36] ga[6]
constexpr double kExpSeries2 = 1e-8, kLogSeries2 = 1e-10, kJrSeries2 = 0.0625;

struct Pose
{
  double R[9];
  double t[3];
};

LSA_HD Pose load(const double* m)
{
  Pose p;
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j) p.R[i * 3 + j] = m[i * 4 + j];
    p.t[i] = m[i * 4 + 3];
  }
  return p;
}
LSA_HD void store(const Pose& p, double* m)
{
  for (int i = 0; i < 3; ++i)
  {
    for (int j = 0; j < 3; ++j) m[i * 4 + j] = p.R[i * 3 + j];
    m[i * 4 + 3] = p.t[i];
  }
  m[12] = 0.; m[13] = 0.; m[14] = 0.; m[15] = 1.;
}

// C = A B, C = A^T B, C = A B^T (3x3)
LSA_HD void mul3(const double* A, const double* B, double* C)
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j];
}
LSA_HD void tmul3(const double* A, const double* B, double* C)
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i] * B[j] + A[3 + i] * B[3 + j]) + A[6 + i] * B[6 + j];
}
LSA_HD void mult3(const double* A, const double* B, double* C)
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = (A[i * 3] * B[j * 3] + A[i * 3 + 1] * B[j * 3 + 1]) + A[i * 3 + 2] * B[j * 3 + 2];
}
// y = A^T v, y = A v
LSA_HD void tmulv3(const double* A, const double* v, double* y)
{
  for (int i = 0; i < 3; ++i) y[i] = (A[i] * v[0] + A[3 + i] * v[1]) + A[6 + i] * v[2];
}
LSA_HD void mulv3(const double* A, const double* v, double* y)
{
  for (int i = 0; i < 3; ++i) y[i] = (A[i * 3] * v[0] + A[i * 3 + 1] * v[1]) + A[i * 3 + 2] * v[2];
}
// [v]x
LSA_HD void hat(const double* v, double* S)
{
  S[0] = 0.;    S[1] = -v[2]; S[2] = v[1];
  S[3] = v[2];  S[4] = 0.;    S[5] = -v[0];
  S[6] = -v[1]; S[7] = v[0];  S[8] = 0.;
}
// I + a [phi]x + b [phi]x^2
LSA_HD void rodrigues(const double* phi, double a, double b, double* R)
{
  double S[9], S2[9];
  hat(phi, S);
  mul3(S, S, S2);
  for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1. : 0.) + (a * S[i] + b * S2[i]);
}

LSA_HD void so3_exp(const double* phi, double* R)
{
  const double t2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
  double a, b;
  if (t2 < kExpSeries2)
  {
    a = 1. - t2 / 6.;
    b = 0.5 - t2 / 24.;
  }
  else
  {
    const double th = __builtin_sqrt(t2);
    const double sh = lsa_sin(0.5 * th);
    a = lsa_sin(th) / th;
    b = (2. * sh * sh) / t2;
  }
  rodrigues(phi, a, b, R);
}

// Eigen::Quaternion(Matrix3d) for a trace <= 0 with I the largest diagonal element
template <int I> LSA_HD void quat_largest(const double* R, double* q)
{
  constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
  double t = __builtin_sqrt(((R[I * 4] - R[J * 4]) - R[K * 4]) + 1.0);
  q[1 + I] = 0.5 * t;
  t = 0.5 / t;
  q[0] = (R[K * 3 + J] - R[J * 3 + K]) * t;
  q[1 + J] = (R[J * 3 + I] + R[I * 3 + J]) * t;
  q[1 + K] = (R[K * 3 + I] + R[I * 3 + K]) * t;
}
LSA_HD void so3_log(const double* R, double* phi)
{
  double q[4];  // w x y z
  double t = (R[0] + R[4]) + R[8];
  if (t > 0.0)
  {
    t = __builtin_sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (R[7] - R[5]) * t;
    q[2] = (R[2] - R[6]) * t;
    q[3] = (R[3] - R[1]) * t;
  }
  else if (R[0] >= R[4] && R[0] >= R[8]) quat_largest<0>(R, q);
  else if (R[4] >= R[8]) quat_largest<1>(R, q);
  else quat_largest<2>(R, q);
  if (q[0] < 0.) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const double n2 = (q[1] * q[1] + q[2] * q[2]) + q[3] * q[3];
  double k;
  if (n2 < kLogSeries2)
    k = (2. / q[0]) * (1. - n2 / (3. * (q[0] * q[0])));
  else
  {
    const double n = __builtin_sqrt(n2);
    k = (2. * lsa_atan2(n, q[0])) / n;
  }
  phi[0] = k * q[1]; phi[1] = k * q[2]; phi[2] = k * q[3];
}

// c(theta) of Jr^-1, from theta^2
LSA_HD double jr_inv_coeff(double t2)
{
  if (t2 < kJrSeries2)
    return 1. / 12. + t2 * (1. / 720. + t2 * (1. / 30240. + t2 * (1. / 1209600. + t2 * (1. / 47900160. + t2 * (691. / 1307674368000.)))));
  const double h = 0.5 * __builtin_sqrt(t2);
  return (1. - (h * lsa_cos(h)) / lsa_sin(h)) / t2;
}
LSA_HD void jr_inv(const double* phi, double* J)
{
  const double t2 = (phi[0] * phi[0] + phi[1] * phi[1]) + phi[2] * phi[2];
  rodrigues(phi, 0.5, jr_inv_coeff(t2), J);
}

LSA_HD Pose retract(const Pose& p, const double* delta)
{
  Pose r;
  double Rr[3], E[9];
  mulv3(p.R, delta, Rr);
  for (int i = 0; i < 3; ++i) r.t[i] = p.t[i] + Rr[i];
  so3_exp(delta + 3, E);
  mul3(p.R, E, r.R);
  return r;
}

// e[6], A[36], B[36] of one edge (6x6 row-major)
LSA_HD void edge_eval(const Pose& Pi, const Pose& Pj, const Pose& Z, double* e, double* A, double* B)
{
  double dt[3], d[3], Rij[9], RE[9], dz[3], J[9], S[9], M[9];
  for (int k = 0; k < 3; ++k) dt[k] = Pj.t[k] - Pi.t[k];
  tmulv3(Pi.R, dt, d);
  tmul3(Pi.R, Pj.R, Rij);
  tmul3(Z.R, Rij, RE);
  for (int k = 0; k < 3; ++k) dz[k] = d[k] - Z.t[k];
  tmulv3(Z.R, dz, e);
  so3_log(RE, e + 3);
  jr_inv(e + 3, J);
  for (int k = 0; k < 36; ++k) { A[k] = 0.; B[k] = 0.; }
  hat(d, S);
  tmul3(Z.R, S, M);  // Rz^T [d]x
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
    {
      A[r * 6 + c] = -Z.R[c * 3 + r];
      A[r * 6 + 3 + c] = M[r * 3 + c];
      B[r * 6 + c] = RE[r * 3 + c];
      B[(3 + r) * 6 + 3 + c] = J[r * 3 + c];
    }
  mult3(J, Rij, M);  // J Rij^T
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) A[(3 + r) * 6 + 3 + c] = -M[r * 3 + c];
}

// C = A B, C = A^T B (6x6), y = A v, y = A^T v: inner index ascending from the first product
LSA_HD void mul6(const double* A, const double* B, double* C)
{
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
    {
      double s = A[i * 6] * B[j];
      for (int k = 1; k < 6; ++k) s += A[i * 6 + k] * B[k * 6 + j];
      C[i * 6 + j] = s;
    }
}
LSA_HD void tmul6(const double* A, const double* B, double* C)
{
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
    {
      double s = A[i] * B[j];
      for (int k = 1; k < 6; ++k) s += A[k * 6 + i] * B[k * 6 + j];
      C[i * 6 + j] = s;
    }
}
LSA_HD void mulv6(const double* A, const double* v, double* y)
{
  for (int i = 0; i < 6; ++i)
  {
    double s = A[i * 6] * v[0];
    for (int k = 1; k < 6; ++k) s += A[i * 6 + k] * v[k];
    y[i] = s;
  }
}
LSA_HD void tmulv6(const double* A, const double* v, double* y)
{
  for (int i = 0; i < 6; ++i)
  {
    double s = A[i] * v[0];
    for (int k = 1; k < 6; ++k) s += A[k * 6 + i] * v[k];
    y[i] = s;
  }
}
LSA_HD double dot6(const double* a, const double* b)
{
  double s = a[0] * b[0];
  for (int k = 1; k < 6; ++k) s += a[k] * b[k];
  return s;
}

// the block record and chi2 of an edge from e, A, B and its information
LSA_HD void edge_blocks(const double* e, const double* A, const double* B, const double* Om, double* blk, double* chi2)
{
  double OA[36], OB[36], Oe[6];
  mul6(Om, A, OA);
  mul6(Om, B, OB);
  mulv6(Om, e, Oe);
  tmul6(A, OA, blk);
  tmul6(A, OB, blk + 36);
  tmul6(B, OB, blk + 72);
  tmulv6(A, Oe, blk + 108);
  tmulv6(B, Oe, blk + 114);
  *chi2 = dot6(e, Oe);
}
// everything of one edge: e[6], blk[kEdgeBlock], chi2
LSA_HD void linearize_edge(const double* poses16, const lsa_pgo_edge_t& ed, double* e, double* blk, double* chi2)
{
  double A[36], B[36];
  edge_eval(load(poses16 + 16 * (long long)ed.from), load(poses16 + 16 * (long long)ed.to), load(ed.relative), e, A, B);
  edge_blocks(e, A, B, ed.information, blk, chi2);
}
// chi2 alone (a candidate's cost)
LSA_HD double edge_chi2(const double* poses16, const lsa_pgo_edge_t& ed)
{
  double e[6], A[36], B[36], Oe[6];
  edge_eval(load(poses16 + 16 * (long long)ed.from), load(poses16 + 16 * (long long)ed.to), load(ed.relative), e, A, B);
  mulv6(ed.information, e, Oe);
  return dot6(e, Oe);
}

// e[3] and A[18] (3x6 row-major) of one prior: the measured position g on pose Pi behind the offset O
LSA_HD void prior_eval(const Pose& Pi, const Pose& O, const double* g, double* e, double* A)
{
  double dt[3], d[3], dz[3], S[9], M[9];
  for (int k = 0; k < 3; ++k) dt[k] = g[k] - Pi.t[k];
  tmulv3(Pi.R, dt, d);
  for (int k = 0; k < 3; ++k) dz[k] = d[k] - O.t[k];
  tmulv3(O.R, dz, e);
  hat(d, S);
  tmul3(O.R, S, M);  // Ro^T [d]x
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
    {
      A[r * 6 + c] = -O.R[c * 3 + r];
      A[r * 6 + 3 + c] = M[r * 3 + c];
    }
}
// the block record and chi2 of a prior from e, A and its information
LSA_HD void prior_blocks(const double* e, const double* A, const double* Om, double* blk, double* chi2)
{
  double OA[18], Oe[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 6; ++j) OA[i * 6 + j] = (Om[i * 3] * A[j] + Om[i * 3 + 1] * A[6 + j]) + Om[i * 3 + 2] * A[12 + j];
  mulv3(Om, e, Oe);
  for (int i = 0; i < 6; ++i)
  {
    for (int j = 0; j < 6; ++j) blk[i * 6 + j] = (A[i] * OA[j] + A[6 + i] * OA[6 + j]) + A[12 + i] * OA[12 + j];
    blk[36 + i] = (A[i] * Oe[0] + A[6 + i] * Oe[1]) + A[12 + i] * Oe[2];
  }
  *chi2 = (e[0] * Oe[0] + e[1] * Oe[1]) + e[2] * Oe[2];
}
// everything of one prior: e[3], blk[kPriorBlock], chi2
LSA_HD void linearize_prior(const double* poses16, const lsa_pgo_prior_t& pr, const Pose& O, double* e, double* blk, double* chi2)
{
  double A[18];
  prior_eval(load(poses16 + 16 * (long long)pr.pose), O, pr.position, e, A);
  prior_blocks(e, A, pr.information, blk, chi2);
}
// chi2 alone (a candidate's cost)
LSA_HD double prior_chi2(const double* poses16, const lsa_pgo_prior_t& pr, const Pose& O)
{
  double e[3], A[18], Oe[3];
  prior_eval(load(poses16 + 16 * (long long)pr.pose), O, pr.position, e, A);
  mulv3(pr.information, e, Oe);
  return (e[0] * Oe[0] + e[1] * Oe[1]) + e[2] * Oe[2];
}

// ROBUST LOSS: rho(s) and w = rho'(s) at scale c (the table in the opening comment, operation by operation)
LSA_HD void robust_rho(int loss, double c, double s, double* rho, double* w)
{
  const double c2 = c * c;
  if (loss == LSA_PGO_LOSS_HUBER)
  {
    if (s > c2)
    {
      const double r = __builtin_sqrt(s);
      *rho = (2. * c) * r - c2;
      *w = c / r;
      return;
    }
  }
  else if (loss == LSA_PGO_LOSS_GEMAN_MCCLURE)
  {
    const double d = c2 + s;
    const double q = c2 / d;
    *rho = (c2 * s) / d;
    *w = q * q;
    return;
  }
  else if (loss == LSA_PGO_LOSS_TUKEY)
  {
    if (s > c2)
    {
      *rho = c2 / 3.;
      *w = 0.;
      return;
    }
    const double v = 1. - s / c2;
    *rho = (s / 3.) * ((1. + v) + v * v);
    *w = v * v;
    return;
  }
  *rho = s;
  *w = 1.;
}
// A robustified constraint's record.  The definition is blk[t] = w * blk[t] for t ascending after the record is formed; each
// element is one product of w and the finished sum, so it is formed here as the sum leaves the registers (the device writes
// the 960 bytes once and never reads them back): the same bits.
LSA_HD void tmul6_scaled(const double* A, const double* B, double w, double* C)
{
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j)
    {
      double s = A[i] * B[j];
      for (int k = 1; k < 6; ++k) s += A[k * 6 + i] * B[k * 6 + j];
      C[i * 6 + j] = w * s;
    }
}
LSA_HD void tmulv6_scaled(const double* A, const double* v, double w, double* y)
{
  for (int i = 0; i < 6; ++i)
  {
    double s = A[i] * v[0];
    for (int k = 1; k < 6; ++k) s += A[k * 6 + i] * v[k];
    y[i] = w * s;
  }
}
// everything of one edge under a loss: e[6], blk[kEdgeBlock] (times w), the raw chi2, rho, w.  loss NONE (an unmasked edge
// is handed NONE): rho = chi2 and w = 1, and a product with 1 is its other factor: linearize_edge's bits
LSA_HD void linearize_edge_robust(const double* poses16, const lsa_pgo_edge_t& ed, int loss, double c, double* e, double* blk, double* chi2, double* rho, double* w)
{
  double A[36], B[36], OA[36], OB[36], Oe[6], ev[6], rv, wv;
  edge_eval(load(poses16 + 16 * (long long)ed.from), load(poses16 + 16 * (long long)ed.to), load(ed.relative), ev, A, B);
  mulv6(ed.information, ev, Oe);
  const double s = dot6(ev, Oe);
  robust_rho(loss, c, s, &rv, &wv);  // NONE: rho = s, w = 1
  mul6(ed.information, A, OA);
  mul6(ed.information, B, OB);
  tmul6_scaled(A, OA, wv, blk);
  tmul6_scaled(A, OB, wv, blk + 36);
  tmul6_scaled(B, OB, wv, blk + 72);
  tmulv6_scaled(A, Oe, wv, blk + 108);
  tmulv6_scaled(B, Oe, wv, blk + 114);
  for (int t = 0; t < 6; ++t) e[t] = ev[t];
  *chi2 = s;
  *rho = rv;
  *w = wv;
}
// a candidate's cost value of one edge, and its weight (the verdict)
LSA_HD double edge_rho(const double* poses16, const lsa_pgo_edge_t& ed, int loss, double c, double* chi2, double* w)
{
  double rho;
  const double s = edge_chi2(poses16, ed);
  *chi2 = s;
  if (loss == LSA_PGO_LOSS_NONE) { *w = 1.; return s; }
  robust_rho(loss, c, s, &rho, w);
  return rho;
}
// the same of one prior
LSA_HD void linearize_prior_robust(const double* poses16, const lsa_pgo_prior_t& pr, const Pose& O, int loss, double c, double* e, double* blk, double* chi2, double* rho,
                                   double* w)
{
  double b[kPriorBlock], s, rv, wv = 1.;
  linearize_prior(poses16, pr, O, e, b, &s);
  rv = s;
  if (loss != LSA_PGO_LOSS_NONE)
  {
    robust_rho(loss, c, s, &rv, &wv);
    for (int t = 0; t < kPriorBlock; ++t) b[t] = wv * b[t];
  }
  for (int t = 0; t < kPriorBlock; ++t) blk[t] = b[t];
  *chi2 = s;
  *rho = rv;
  *w = wv;
}
LSA_HD double prior_rho(const double* poses16, const lsa_pgo_prior_t& pr, const Pose& O, int loss, double c, double* chi2, double* w)
{
  double rho;
  const double s = prior_chi2(poses16, pr, O);
  *chi2 = s;
  if (loss == LSA_PGO_LOSS_NONE) { *w = 1.; return s; }
  robust_rho(loss, c, s, &rho, w);
  return rho;
}
// lsa_pgo_robust_t within its limits
LSA_HD bool robust_ok(const lsa_pgo_robust_t& r)
{
  return r.edge_loss >= 0 && r.edge_loss <= 3 && r.prior_loss >= 0 && r.prior_loss <= 3 &&
         (r.edge_loss == LSA_PGO_LOSS_NONE || (r.edge_scale > 0. && r.edge_scale - r.edge_scale == 0.)) &&
         (r.prior_loss == LSA_PGO_LOSS_NONE || (r.prior_scale > 0. && r.prior_scale - r.prior_scale == 0.));
}

// W P and inv(A) P of rigid poses: what brings a trajectory into the frame of the measured positions and back onto its pose 0
LSA_HD Pose compose(const Pose& W, const Pose& P)
{
  Pose r;
  double Wt[3];
  mul3(W.R, P.R, r.R);
  mulv3(W.R, P.t, Wt);
  for (int k = 0; k < 3; ++k) r.t[k] = Wt[k] + W.t[k];
  return r;
}
LSA_HD Pose inverse_compose(const Pose& A, const Pose& P)
{
  Pose r;
  double dt[3];
  tmul3(A.R, P.R, r.R);
  for (int k = 0; k < 3; ++k) dt[k] = P.t[k] - A.t[k];
  tmulv3(A.R, dt, r.t);
  return r;
}

// The incidence lists of the poses (CSR, ascending edge index) and, per pose, its couplings beyond the chain: entry k of
// row i names the edge and whether pose i is its `to` end (the block is then Hab^T).
struct Graph
{
  const int* row_start;   // [n + 1]
  const int* inc;         // [2 m] edge indices
  const int* loop_start;  // [n + 1]
  const int* loop_edge;   // edge index * 2 + (1 when pose i is the edge's `to`)
  const int* loop_col;    // the other pose
  const int* prior_start; // [n + 1] the priors of the poses, ascending prior index (all zero without priors)
  const int* prior_of;    // prior indices
};

// Row i of the assembly at lambda: D (damped), dg = diag(H) (undamped), g, L = block (i, i-1), U = block (i, i+1)
LSA_HD void assemble_row(int i, int n, const unsigned char* fixed, const Graph& G, const lsa_pgo_edge_t* edges, const double* blocks, const double* pblocks, double lambda,
                         double* D, double* dg, double* g, double* L, double* U)
{
  for (int k = 0; k < 36; ++k) { D[k] = 0.; L[k] = 0.; U[k] = 0.; }
  for (int k = 0; k < 6; ++k) { g[k] = 0.; dg[k] = 0.; }
  if (fixed[i])
  {
    for (int k = 0; k < 6; ++k) D[k * 7] = 1.;
    return;
  }
  bool first = true, firstL = true, firstU = true;
  for (int a = G.row_start[i]; a < G.row_start[i + 1]; ++a)
  {
    const int ei = G.inc[a];
    const lsa_pgo_edge_t& ed = edges[ei];
    const double* blk = blocks + (long long)ei * kEdgeBlock;
    const bool isFrom = ed.from == i;
    const double* Hd = isFrom ? blk : blk + 72;
    const double* gd = isFrom ? blk + 108 : blk + 114;
    for (int k = 0; k < 36; ++k) D[k] = first ? Hd[k] : D[k] + Hd[k];
    for (int k = 0; k < 6; ++k) g[k] = first ? gd[k] : g[k] + gd[k];
    first = false;
    const int other = isFrom ? ed.to : ed.from;
    if (fixed[other] || (other != i - 1 && other != i + 1)) continue;
    double* T = other == i - 1 ? L : U;
    bool& firstT = other == i - 1 ? firstL : firstU;
    const double* Hab = blk + 36;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c)
      {
        const double v = isFrom ? Hab[r * 6 + c] : Hab[c * 6 + r];
        T[r * 6 + c] = firstT ? v : T[r * 6 + c] + v;
      }
    firstT = false;
  }
  for (int a = G.prior_start[i]; a < G.prior_start[i + 1]; ++a)
  {
    const double* blk = pblocks + (long long)G.prior_of[a] * kPriorBlock;
    for (int k = 0; k < 36; ++k) D[k] = first ? blk[k] : D[k] + blk[k];
    for (int k = 0; k < 6; ++k) g[k] = first ? blk[36 + k] : g[k] + blk[36 + k];
    first = false;
  }
  for (int k = 0; k < 6; ++k)
  {
    dg[k] = D[k * 7];
    D[k * 7] = D[k * 7] + lambda * D[k * 7];
  }
  (void)n;
}

// q_i = D_i p_i + L_i p_{i-1} + U_i p_{i+1} + the loop blocks of row i in the order of its list
LSA_HD void spmv_row(int i, int n, const Graph& G, const double* blocks, const double* D, const double* L, const double* U, const double* p, double* q)
{
  double acc[6], y[6];
  mulv6(D + 36LL * i, p + 6LL * i, acc);
  if (i > 0)
  {
    mulv6(L + 36LL * i, p + 6LL * (i - 1), y);
    for (int k = 0; k < 6; ++k) acc[k] += y[k];
  }
  if (i + 1 < n)
  {
    mulv6(U + 36LL * i, p + 6LL * (i + 1), y);
    for (int k = 0; k < 6; ++k) acc[k] += y[k];
  }
  for (int a = G.loop_start[i]; a < G.loop_start[i + 1]; ++a)
  {
    const int code = G.loop_edge[a];
    const double* Hab = blocks + (long long)(code >> 1) * kEdgeBlock + 36;
    const double* pj = p + 6LL * G.loop_col[a];
    if (code & 1) tmulv6(Hab, pj, y);
    else mulv6(Hab, pj, y);
    for (int k = 0; k < 6; ++k) acc[k] += y[k];
  }
  for (int k = 0; k < 6; ++k) q[k] = acc[k];
}

// Cholesky of a symmetric positive definite 6x6 (its lower triangle is read), the operations of SolveSPD (host/lsa_lm.cpp) and
// solve_spd<6> (lsa_device_math.h): divisions by a diagonal element are multiplications by its reciprocal, taken once
struct Chol6
{
  double L[36];
  double rinv[6];
};
LSA_HD bool chol6(const double* A, Chol6& c)
{
  bool ok = true;
  for (int i = 0; i < 36; ++i) c.L[i] = 0.;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j)
    {
      double s = A[i * 6 + j];
      for (int k = 0; k < j; ++k) s -= c.L[i * 6 + k] * c.L[j * 6 + k];
      if (i == j)
      {
        if (!(s > 0.0) || !(s <= 1.79769313486231570815e308)) { ok = false; s = 1.; }
        c.L[i * 6 + i] = __builtin_sqrt(s);
        c.rinv[i] = 1.0 / c.L[i * 6 + i];
      }
      else
        c.L[i * 6 + j] = s * c.rinv[j];
    }
  return ok;
}
LSA_HD void chol6_solve(const Chol6& c, const double* b, double* x)
{
  double y[6];
  for (int i = 0; i < 6; ++i)
  {
    double s = b[i];
    for (int k = 0; k < i; ++k) s -= c.L[i * 6 + k] * y[k];
    y[i] = s * c.rinv[i];
  }
  for (int i = 5; i >= 0; --i)
  {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s -= c.L[k * 6 + i] * x[k];
    x[i] = s * c.rinv[i];
  }
}
// X = M D^-1 for the symmetric D behind c: row r of X solves D x = (row r of M)
LSA_HD void chol6_right(const Chol6& c, const double* M, double* X)
{
  for (int r = 0; r < 6; ++r) chol6_solve(c, M + r * 6, X + r * 6);
}

LSA_HD bool finite_d(double v) { return v - v == 0.; }

// lsa_pgo_params_t within its limits
LSA_HD bool params_ok(const lsa_pgo_params_t& p)
{
  return p.max_iterations >= 0 && p.pcg_max_iter >= 1 && p.pcg_tolerance > 0. && p.pcg_tolerance < 1. && p.initial_lambda > 0. && finite_d(p.initial_lambda) &&
         p.lambda_shrink > 0. && p.lambda_shrink <= 1. && p.lambda_grow > 1. && finite_d(p.lambda_grow) && p.lambda_min >= 0. && p.lambda_max >= p.lambda_min &&
         p.gradient_tolerance >= 0. && p.step_tolerance >= 0. && p.cost_tolerance >= 0. && (p.preconditioner == 0 || p.preconditioner == 1) &&
         (p.odometry_information == 0 || p.odometry_information == 1);
}
}  // namespace pg
}  // namespace lsa
