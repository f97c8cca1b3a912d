// lsa_lm.hip -- LocalOptimizer::Solve (slam_lib/src/LocalOptimizer.cxx:74-102) as ONE launch.
//
// The host-driven loop (host/lsa_lm_loop.cpp) pays a kernel launch and a PCIe round trip per trust-region
// evaluation, ~4 per solve, ~25 per frame.  Here the whole Levenberg-Marquardt loop of Ceres (unpinned
// master >= 2.0 in the reference CI: TukeyLoss a^2/3, ScaledLoss(weight), DENSE_QR on a 6-column
// Jacobian = the 6x6 normal equations, Solver::Options defaults) runs inside one kernel:
//
//   * every block evaluates its share of the residual blocks at the candidate pose (lsa_accum.h) and reduces
//     it in a fixed order to 29 sums;
//   * the blocks exchange those sums through 8-byte {tag, half of a double} granules in device memory, each
//     ONE relaxed agent-scope atomic store / load (MI355X: `sc1`, write-through past the non-coherent per-XCD
//     L2s): tag and payload are one memory object, so no fence, flag or ordering between locations is needed.
//     Two parities of slots: a block can be at most one evaluation ahead of the slowest;
//   * EVERY block folds all partial sums in a fixed order -- 8 partial sums per value over the blocks j, j + 8, ..., then
//     the 8 in order; wavefront j reads the granules of its blocks and sums them itself: no copy of the granules in LDS,
//     one barrier between publishing and the step -- and runs the 6x6 trust-region algebra itself, its first wavefront
//     with a row of the system per lane (lm_step): same inputs, same instructions, same result in every block, so the
//     next candidate needs no broadcast;
//   * block 0 hands pose, summary and the normal equations at the final point to the host through the same
//     kind of granules in coherent host memory.
// The arithmetic of the trust-region step is the host loop's, operation for operation (no FMA contraction, IEEE
// division and square root): given the same sums both take the same decisions.  The sums differ in the last
// bits (more blocks, and sin/cos of the angles come from lsa_pmath.h instead of libm).
// Every spin is bounded: a block that waits too long gives up, the launch drains, the host falls back to the
// host-driven loop and counts it (lsa_ctx::lm_fallbacks).
#include <chrono>
#include <cmath>
#include "lsa_accum.h"
#include "lsa_device_math.h"
#include "lsa_sensor_terms.h"
#include "../../include/lsa_pmath.h"

using namespace lsa;

namespace
{

typedef unsigned long long u64;
#ifndef LSA_RECORD_PREFETCH
#define LSA_RECORD_PREFETCH 1
#endif
constexpr bool kRecordPrefetch = LSA_RECORD_PREFETCH != 0;  // (0: A/B builds)

struct LmParams
{
  RecordSet set;
  double x0[6];
  int two_d;
  int max_iter;
  int min_matches;
  unsigned tag_base;
  int cslots;  // residual blocks per thread kept in LDS between the evaluations
  int give_up_block;    // test hook: this workgroup abandons the exchange at its first evaluation (-1: none)
  const IcpLinkBlock* link;  // not null: the launch was enqueued ahead of its start point (lsa_icp_link) -- x0 comes from there, or nothing is done
  // What this solve leaves for the ICP iteration enqueued behind it (lsa_icp_link; Slam.cxx:907, 940-950 and 1086, 1134-1151):
  // whether it runs at all, the pose its keypoints are searched under, its start point and -- localization -- the undistortion.
  IcpLinkBlock* leave;             // null: nothing is left (no iteration behind this one)
  int link_refine;            // localization with Slam::RefineUndistortion between two iterations
  int motion_from_args;       // the motion within the frame as the loop starts with it: motion0 (first solve of the loop) or motion_dev
  posemath::ScanPoseClock clock;
  Rigid previous_world;       // PreviousTworld
  double motion0[16];         // Time0, Time1, Rot0 (w x y z), Rot1, Trans0, Trans1
  double* motion_dev;         // the same 16 values between the solves of one loop
  // wheel odometer / gravity terms of the localization problem (lsa_set_sensor_terms), by value: a solve enqueued ahead
  // carries the terms of the moment it was enqueued
  lsa_sensor_terms_t sensors;
  int sensors_on;
};

// result layout (doubles): [0..5] pose, [6] initial cost, [7] final cost, [8..36] the 29 sums at the final
// point, [37] successful steps, [38] unsuccessful steps, [39] iterations, [40] evaluations, [41] skipped,
// [42] termination code, [43] matches, [44] failure (a spin ran out)
constexpr int kResPose = 0, kResInitial = 6, kResFinal = 7, kResSums = 8, kResSuccessful = 37, kResUnsuccessful = 38, kResIterations = 39,
              kResEvaluations = 40, kResSkipped = 41, kResCode = 42, kResMatches = 43, kResFailed = 44, kResCount = 45;
static_assert(kResCount <= kLmOut, "result does not fit the mailbox");

// index of H(a, b), a <= b, in the 29 sums (cost, g[6], upper triangle row by row, count)
__device__ __forceinline__ constexpr int hidx(int a, int b) { return 7 + a * 6 - (a * (a - 1)) / 2 + (b - a); }
__device__ __forceinline__ constexpr int hsym(int a, int b) { return a <= b ? hidx(a, b) : hidx(b, a); }

// trust-region state between two evaluations (every block keeps its own copy in LDS: nothing of it is live in registers
// while the residual blocks are evaluated; lm_step loads it into the first wavefront's lanes and lane 0 writes it back)
struct LmState
{
  int cur_buf;             // which of Shared::sums holds the sums at the current point x (the other one takes the next evaluation's)
  double x[6], scale[6], diag[6];
  double radius, decrease_factor, x_norm, model_cost_change, delta_norm, initial_cost;
  int reuse_diagonal, consecutive_invalid, iter;
  int evaluations, successful, unsuccessful, iterations, code, skipped, matches;
};

struct Shared
{
  double wsum[kLmThreads / 64][kAccumVals];
  double part[kAccumVals][8];  // the fold's 8 partial sums per value, a wavefront each
  // The sums over ALL residual blocks, twice: at the current point, and of the evaluation under way / just done.  A step that
  // is accepted makes the second the first by flipping LmState::cur_buf (29 values that one thread no longer copies).
  double sums[2][kAccumVals];
  double Hs[36], gs[6];     // the scaled system at the current point (lm_step: written when a point is accepted, lane a its row)
  double w[6];              // the point to evaluate next
  double rot[39];           // R, dR/drx, dR/dry, dR/drz, t at w
  LmState lm;
  int failed;
  int stop;
  unsigned long long lap[6], tk;  // diagnostics (block 0): evaluate, exchange, fold, step [100 MHz ticks], evaluations, total
  unsigned long long sub[4], st0;  // diagnostics: parts of the step -- decision, scaled system, Cholesky solve, candidate
};

__device__ __forceinline__ double uniform(double v)
{
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// the value another lane of the wavefront holds
__device__ __forceinline__ double lane_value(double v, int lane)
{
  const long long b = __double_as_longlong(v);
  const int lo = __shfl((int)(b & 0xffffffffll), lane), hi = __shfl((int)(b >> 32), lane);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

// the value lane `src` of the wavefront holds (the same src in all lanes: v_readlane), the same value in every lane afterwards
__device__ __forceinline__ double lane_bcast(double v, int src)
{
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src), hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}

__device__ __forceinline__ void lm_lap(Shared& sh, int slot)
{
  if (threadIdx.x == 0)
  {
    const unsigned long long now = wall_clock64();
    sh.lap[slot] += now - sh.tk;
    sh.tk = now;
  }
}

// The sensor terms (lsa_sensor_terms.h) on top of the sums of the evaluation just folded, at sh.w / sh.rot.  Not inlined:
// inlined, its ~80 live doubles raised the kernel's VGPR count (229 -> 242) and SGPR spills (81 -> 114); as a call the
// kernel keeps 229 VGPRs, no scratch memory and the same LDS, and a solve without terms never makes the call.
__device__ __noinline__ void lm_sensor_terms(const lsa_sensor_terms_t* terms, Shared& sh)
{
  sensor_terms_add(*terms, sh.w, sh.rot, sh.rot + 9, sh.rot + 18, sh.rot + 27, true, sh.sums[1 - sh.lm.cur_buf]);
}

// One evaluation at sh.w / sh.rot: sh.sums[1 - cur_buf][] = the 29 sums over ALL residual blocks, identical in every block.
// Returns false when a spin ran out (uniform over the block).  One barrier between publishing the block's sums and the step.
__device__ __forceinline__ bool lm_evaluate(const LmParams& p, unsigned epoch, u64* __restrict__ xchg, Shared& sh, double* __restrict__ cache, bool trace)
{
  {
    RotConst c;
    // the same values in every lane: kept in scalar registers
#pragma unroll
    for (int i = 0; i < 9; ++i) { c.R[i] = uniform(sh.rot[i]); c.dRx[i] = uniform(sh.rot[9 + i]); c.dRy[i] = uniform(sh.rot[18 + i]); c.dRz[i] = uniform(sh.rot[27 + i]); }
#pragma unroll
    for (int i = 0; i < 3; ++i) c.t[i] = uniform(sh.rot[36 + i]);
    double acc[kAccumVals];
#pragma unroll
    for (int v = 0; v < kAccumVals; ++v) acc[v] = 0.;
    const unsigned long long e0 = trace ? wall_clock64() : 0ull;
    accumulate_records_cached(p.set, c, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, cache, p.cslots, p.cslots * kLmThreads, epoch == 1, kRecordPrefetch && p.cslots > 0 ? 1 : 0, acc);
    const unsigned long long e1 = trace ? wall_clock64() : 0ull;
    int slot;
    const double total = wave_reduce_accum(acc, slot);  // this lane's one value of the 29, summed over the wavefront
    if (trace && threadIdx.x == 0) { sh.lap[4] += e1 - e0; }
    if ((threadIdx.x & 1) == 0 && slot < kAccumVals) sh.wsum[threadIdx.x >> 6][slot] = total;
  }
  if (threadIdx.x == 0) sh.failed = 0;
  __syncthreads();
  if (trace) lm_lap(sh, 0);
  const unsigned tag = p.tag_base + epoch;
  const int nb = gridDim.x;
  u64* slots = xchg + (size_t)(epoch & 1u) * kLmBlocksMax * kMailboxStride;
  if (threadIdx.x < 2 * kAccumVals)
  {
    const int v = threadIdx.x >> 1, half = threadIdx.x & 1;
    double r = sh.wsum[0][v];
#pragma unroll
    for (int w = 1; w < kLmThreads / 64; ++w) r += sh.wsum[w][v];  // ((w0 + w1) + w2) + ...
    const u64 bits = (u64)__double_as_longlong(r);
    const unsigned word = half ? (unsigned)(bits >> 32) : (unsigned)(bits & 0xffffffffull);
    __hip_atomic_store(slots + (size_t)blockIdx.x * kMailboxStride + threadIdx.x, ((u64)tag << 32) | word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // gather and fold, straight from the granules.  The fold's order is fixed: 8 partial sums per value, partial j over the
  // blocks b = j, j + 8, ... in ascending b starting from 0, then the 8 in the order ((p0 + p1) + p2) + ...  Wavefront j
  // of the 8 works out partial j of all 29 values: its lane s < 58 loads granule s of its blocks -- one load of a wavefront
  // is one block's 464 contiguous bytes, kFoldBatch of them in flight together -- again and again until every tag
  // matches; the even lane 2v takes the upper half of value v from its neighbour (a DPP move) and sums.  Only the 8 x 29
  // partial sums pass through LDS, and the one barrier of the exchange stands behind them.
  static_assert(kLmThreads / 64 == 8, "a wavefront per partial sum of the fold");
  bool failed = (int)blockIdx.x == p.give_up_block;  // (test hook: as if this workgroup had waited too long)
  {
    constexpr int kFoldBatch = 8;
    const int j = threadIdx.x >> 6, s = threadIdx.x & 63;
    const bool loads = s < 2 * kAccumVals;
    const u64* mine = slots + s;
    double sum = 0.;
    const unsigned long long t0 = wall_clock64();
    unsigned spins = 0;
    for (int b0 = j; b0 < nb; b0 += 8 * kFoldBatch)
    {
      u64 x[kFoldBatch];
#pragma unroll
      for (int k = 0; k < kFoldBatch; ++k) x[k] = 0ull;
      while (loads && !failed)
      {
#pragma unroll
        for (int k = 0; k < kFoldBatch; ++k)
          if (b0 + 8 * k < nb) x[k] = __hip_atomic_load(mine + (size_t)(b0 + 8 * k) * kMailboxStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool ok = true;
#pragma unroll
        for (int k = 0; k < kFoldBatch; ++k)
          if (b0 + 8 * k < nb && (unsigned)(x[k] >> 32) != tag) ok = false;
        if (ok) break;
        // 100 MHz clock: 20 ms without the other blocks' sums (they are not resident, or gave up themselves)
        if ((++spins & 15u) == 0 && wall_clock64() - t0 > 2000000ull) { failed = true; break; }
        __builtin_amdgcn_s_sleep(2);
      }
      // all lanes again: lane 2v + 1 holds the upper half of what lane 2v holds the lower half of (quad_perm [1, 1, 3, 3])
#pragma unroll
      for (int k = 0; k < kFoldBatch; ++k)
      {
        const unsigned lo = (unsigned)(x[k] & 0xffffffffull);
        const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)lo, 0xF5, 0xf, 0xf, false);
        if (b0 + 8 * k < nb) sum += __longlong_as_double((long long)(((u64)hi << 32) | lo));
      }
    }
    if (trace) lm_lap(sh, 1);
    // (a lane that gave up, or whose neighbour did, holds no sum -- and no sum is used then)
    if (loads && (s & 1) == 0) sh.part[s >> 1][j] = sum;
  }
  if (failed) atomicOr(&sh.failed, 1);
  __syncthreads();
  if (sh.failed) return false;
  // the 8 partial sums of a value in order, by the first wavefront -- the one that reads the sums next (the sensor terms,
  // lm_step: the LDS operations of one wavefront are served in order), so no barrier follows
  if (threadIdx.x < kAccumVals)
  {
    double r = sh.part[threadIdx.x][0];
#pragma unroll
    for (int i = 1; i < 8; ++i) r += sh.part[threadIdx.x][i];
    sh.sums[1 - sh.lm.cur_buf][threadIdx.x] = r;
  }
  if (threadIdx.x < 64) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  // the sensor terms on top of the fold, the same arithmetic in every block; lane 0 of the first wavefront, which is the
  // one that reads the sums next (lm_step: its LDS operations are served in order).  One uniform branch.
  if (p.sensors_on && threadIdx.x == 0)
  {
    // the callee reads the terms straight from the kernel arguments (LmParams is the first one): taking the address of
    // `p` would copy all of it to scratch memory
    const char* args = (const char*)__builtin_amdgcn_kernarg_segment_ptr();
    const lsa_sensor_terms_t* terms = reinterpret_cast<const lsa_sensor_terms_t*>(args + offsetof(LmParams, sensors));
    lm_sensor_terms(terms, sh);
  }
  if (trace) lm_lap(sh, 2);
  return true;
}

enum LmCode
{
  kCodeNone = 0, kCodeNotEnoughMatches, kCodeGradient0, kCodeMaxIterations, kCodeGradient, kCodeMinRadius, kCodeInvalidSteps, kCodeParameterTolerance,
  kCodeFunctionTolerance
};

// sh.w = the point to evaluate next, sh.rot = rotation and derivatives there (CeresCostFunctions.h:67-79).  The first
// wavefront runs it, all lanes; every lane holds the point (the same six values in all of them: lm_step works the
// candidate out that way), so the six lanes that work out the three cosines and three sines -- a few hundred dependent
// instructions each, side by side instead of one lane six times -- take their angle from their own registers and do not
// wait for sh.w to make the round trip through LDS.
// (The point comes by value: a lane's choice among values is a select, among the elements of an array in memory it would
// be an indexed load from scratch memory.)
__device__ __forceinline__ void finish_point(Shared& sh, double x, double y, double z, double rx, double ry, double rz)
{
  const double w[6] = {x, y, z, rx, ry, rz};
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));  // (as in lm_step: no lane masks kept in scalar registers across the evaluation)
  const int k = lane < 6 ? lane % 3 : 0;
  const double angle = k == 0 ? rx : (k == 1 ? ry : rz);
  const double v = lane < 3 ? lsa_cos(angle) : lsa_sin(angle);
  const double cx = lane_bcast(v, 0), cy = lane_bcast(v, 1), cz = lane_bcast(v, 2);
  const double sx = lane_bcast(v, 3), sy = lane_bcast(v, 4), sz = lane_bcast(v, 5);
  if (lane == 0)
  {
    double R[9], dRx[9], dRy[9], dRz[9];
    rotation_and_derivatives(cx, sx, cy, sy, cz, sz, R, dRx, dRy, dRz);
#pragma unroll
    for (int i = 0; i < 9; ++i) { sh.rot[i] = R[i]; sh.rot[9 + i] = dRx[i]; sh.rot[18 + i] = dRy[i]; sh.rot[27 + i] = dRz[i]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) sh.rot[36 + i] = w[i];
#pragma unroll
    for (int a = 0; a < 6; ++a) sh.w[a] = w[a];
  }
}

// What the trust-region loop of host/lsa_lm_loop.cpp (LocalOptimizer::Solve) does between two evaluations, N active
// parameters: all 6, or (x, y, rz) in 2D mode (SubsetParameterization(6, {2, 3, 4}), LocalOptimizer.cxx:89-90).
// In: sh.sums[1 - cur_buf] = the sums at sh.w (the start point when first, a candidate afterwards).  Out: cand = the next
// candidate, or true = the solve is over (sh.stop says so to the other wavefronts behind the barrier).
//
// The first wavefront runs it, ALL lanes through the same instructions.  What is one value -- the decision on the
// candidate, the radius, the pivots, the step, the next candidate -- every lane works out for itself from the same
// operands (no more instructions than one lane alone would issue, and nothing to hand round afterwards); what is a row
// of the 6 x 6 system belongs to lane a < N, and lane N carries the right-hand side as one more row:
//   * the Jacobi scales 1 / (1 + sqrt(H_aa)), the row of the scaled system, the clamped diagonal and M_aa: lane a;
//   * the Cholesky factor column by column: the pivot goes round (v_readlane), lane i > j works out L_ij, and lane N the
//     forward substitution's y_j by the same formula -- every entry subtracts its products in the order k = 0, 1, ...
//     (each as soon as column k exists), and multiplies by the reciprocal of the pivot, as solve_spd<N> does;
//   * back substitution row by row (its sums run over k ascending while x_k arrive descending: nothing to spread);
//   * the rows t_a = sum_b Hs_ab step_b of the model's cost change: lane a; s.g and s.Hs are added in order.
// The scaled system of the current point stays in sh.Hs / sh.gs from the accepted step (or the start) that made it; a
// rejected step only loads it.  The system of the point just evaluated is formed before it is known whether the
// candidate is accepted -- its loads and products are independent of the decision's divisions and run in their shadow --
// and stored only if it is.  Everything the step reads from LDS is loaded at its head, one latency for all of it.
// The arithmetic of every value is the host loop's, operation for operation, every sum in the host's order.
// The orders are a contract (tests/lm_step_cases.py states the loop independently and compares bit patterns; device: this
// step through lsa_selftest_lm_step, host: host/lsa_lm_loop.cpp through lsa_selftest_lm_host): Hs_ab = (H_ab s_a) s_b and
// gs_a = g_a s_a; M_aa = Hs_aa + D_a / radius; every entry of the factor subtracts its products with k ascending and is
// multiplied by the reciprocal of the pivot, 1 / sqrt(d); both substitutions subtract with k ascending; t_a = sum_b Hs_ab
// step_b, s.g = sum_a step_a gs_a and s.Hs = sum_a step_a t_a from 0 in index order; the change is -s.g - 0.5 s.Hs;
// cand_a = x_a + step_a s_a, |step|^2 = sum (x_a - cand_a)^2 in index order.
template <int N> __device__ __forceinline__ constexpr int lm_act(int a) { return N == 6 ? a : (a == 2 ? 5 : a); }
// the gradient tolerance: max |g_a| <= tolerance, said entry by entry -- a gradient with a NaN in it has not converged,
// wherever the NaN stands (a maximum by comparisons loses it again at the next entry)
template <int N>
__device__ __forceinline__ bool lm_grad_below(const double g[N], double tolerance)
{
  bool below = true;
#pragma unroll
  for (int a = 0; a < N; ++a) below = below && __builtin_fabs(g[a]) <= tolerance;
  return below;
}
template <int N>
__device__ __forceinline__ double lm_x_norm(const double x[6])
{
  double s = 0;
#pragma unroll
  for (int a = 0; a < N; ++a) s += x[lm_act<N>(a)] * x[lm_act<N>(a)];
  return __builtin_sqrt(s);
}
template <int N>
__device__ __forceinline__ bool lm_step(const LmParams& p, Shared& sh, bool first, double cand[6])
{
  const double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;
  const double min_relative_decrease = 1e-3, max_radius = 1e16, min_trust_region_radius = 1e-32;
  const double min_diagonal = 1e-6, max_diagonal = 1e32;
  const int max_consecutive_invalid = 5;
  // (The lane number passes through an empty asm statement: the lane masks made from it -- a pair of scalar registers
  // for every `row == j` -- would otherwise be worked out once, ahead of the loop over the evaluations, and stay live
  // through the residual blocks, whose rotation constants then no longer fit the scalar registers.)
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));
  const bool l0 = lane == 0;
  const int row = lane < N ? lane : 0;  // (the lanes behind the rows work row 0 out again: nobody reads what they hold)
  const int fr = N == 6 ? row : (row == 2 ? 5 : row);  // lm_act<N>(row)
  LmState& lm = sh.lm;
  unsigned long long t0 = sh.st0;  // tracing (block 0): the clock at the head of the part under way
  auto stamp = [&](int part) {
    if (t0 && l0) { const unsigned long long n = wall_clock64(); sh.sub[part] += n - t0; t0 = n; }
  };

  // ---- everything the step reads
  int cur_buf = lm.cur_buf;
  const double* tot = sh.sums[1 - cur_buf];  // at the point just evaluated
  const double* old = sh.sums[cur_buf];      // at the current point
  const double tot_cost = tot[0], old_cost = old[0], tot_count = tot[28];
  double tot_g[N], old_g[N], tot_row[N], kept_row[N], kept_gs[N], scale[N], x_old[6], x_w[6];
#pragma unroll
  for (int a = 0; a < N; ++a)
  {
    const int fb = lm_act<N>(a);
    const int lo = fr <= fb ? fr : fb, hi = fr <= fb ? fb : fr;
    tot_g[a] = tot[1 + fb];
    old_g[a] = old[1 + fb];
    tot_row[a] = tot[7 + lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)];  // hsym(fr, fb)
    kept_row[a] = sh.Hs[row * N + a];
    kept_gs[a] = sh.gs[a];
    scale[a] = lm.scale[a];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) { x_old[a] = lm.x[a]; x_w[a] = sh.w[a]; }
  double scale_row = lm.scale[row], diag_row = lm.diag[row];
  double radius = lm.radius, decrease_factor = lm.decrease_factor, x_norm = lm.x_norm, model_cost_change = lm.model_cost_change, delta_norm = lm.delta_norm;
  int reuse_diagonal = lm.reuse_diagonal, consecutive_invalid = lm.consecutive_invalid, iter = lm.iter;
  int successful = lm.successful, unsuccessful = lm.unsuccessful, evaluations = lm.evaluations;
  double tot_diag = tot_row[0];  // H(fr, fr)
#pragma unroll
  for (int b = 1; b < N; ++b)
    if (row == b) tot_diag = tot_row[b];

  // ---- what became of the candidate; use_tot: the sums just folded are the current ones from now on
  bool use_tot;
  if (first)
  {
    const int matches = (int)tot_count;
    if (l0) lm.matches = matches;
    if (matches < p.min_matches)
    {
      if (l0) { lm.skipped = 1; lm.code = kCodeNotEnoughMatches; sh.stop = 1; }
      return true;
    }
    use_tot = true;  // the sums at the start point are the current ones
    successful = 1;  // iteration 0 is reported as a successful step by Ceres
    scale_row = 1.0 / (1.0 + __builtin_sqrt(tot_diag));  // Jacobi scaling, once
#pragma unroll
    for (int a = 0; a < N; ++a) scale[a] = lane_bcast(scale_row, a);
    if (lane < N) lm.scale[lane] = scale_row;
    if (l0) { lm.initial_cost = tot_cost; lm.cur_buf = cur_buf ^ 1; lm.successful = 1; }
    if (lm_grad_below<N>(tot_g, gradient_tolerance))
    {
      if (l0) { lm.code = kCodeGradient0; sh.stop = 1; }
      return true;
    }
    x_norm = lm_x_norm<N>(x_old);  // (sh.w is the start point, and so is LmState::x)
  }
  else
  {
    // parameter / function tolerance terminate WITHOUT taking the candidate step
    if (delta_norm <= parameter_tolerance * (x_norm + parameter_tolerance))
    {
      if (l0) { lm.code = kCodeParameterTolerance; sh.stop = 1; }
      return true;
    }
    const double cost_change = old_cost - tot_cost;
    if (__builtin_fabs(cost_change) <= function_tolerance * old_cost)
    {
      if (l0) { lm.code = kCodeFunctionTolerance; sh.stop = 1; }
      return true;
    }
    const double relative_decrease = cost_change / model_cost_change;
    use_tot = relative_decrease > min_relative_decrease;
    if (use_tot)
    {
      // cost AND Jacobian were evaluated at the candidate (Ceres evaluates the Jacobian again on acceptance, at the
      // same point: same arithmetic, one evaluation less): its sums become the current ones
      x_norm = lm_x_norm<N>(x_w);
      ++successful;
      const double t = 2.0 * relative_decrease - 1.0;
      const double q = 1.0 - t * t * t;
      const double d = (1.0 / 3.0) < q ? q : (1.0 / 3.0);  // std::max(1.0 / 3.0, q)
      const double r = radius / d;
      radius = r < max_radius ? r : max_radius;            // std::min(max_radius, r)
      decrease_factor = 2.0;
      reuse_diagonal = 0;
    }
    else
    {
      ++unsuccessful;
      radius /= decrease_factor; decrease_factor *= 2.0; reuse_diagonal = 1;
    }
  }
  if (use_tot) cur_buf ^= 1;
  stamp(0);

  // ---- the normal equations at the current point, scaled: lane a its row, every lane the gradient
  double x[6], g[N], Hrow[N], gs[N];
#pragma unroll
  for (int a = 0; a < 6; ++a) x[a] = use_tot ? x_w[a] : x_old[a];
#pragma unroll
  for (int a = 0; a < N; ++a)
  {
    g[a] = use_tot ? tot_g[a] : old_g[a];
    const double h = tot_row[a] * scale_row * scale[a];
    const double gsa = tot_g[a] * scale[a];
    Hrow[a] = use_tot ? h : kept_row[a];
    gs[a] = use_tot ? gsa : kept_gs[a];
  }
  if (use_tot)
  {
    // kept for the rejected steps that may follow
    if (lane < N)
    {
#pragma unroll
      for (int a = 0; a < N; ++a) sh.Hs[lane * N + a] = Hrow[a];
    }
    if (l0)
    {
#pragma unroll
      for (int a = 0; a < N; ++a) sh.gs[a] = gs[a];
    }
  }
  const bool grad_below = lm_grad_below<N>(g, gradient_tolerance);
  double Hdiag = Hrow[0];  // Hs(row, row)
#pragma unroll
  for (int b = 1; b < N; ++b)
    if (row == b) Hdiag = Hrow[b];

  // ---- the damped solve and the next candidate; again with a smaller radius while the step is invalid
  int code = kCodeNone;
  while (true)
  {
    if (iter >= p.max_iter) { code = kCodeMaxIterations; break; }
    if (grad_below) { code = kCodeGradient; break; }
    if (radius < min_trust_region_radius) { code = kCodeMinRadius; break; }
    ++iter;
    if (!reuse_diagonal)
    {
      const double lo = Hdiag < min_diagonal ? min_diagonal : Hdiag;  // std::max(h, min_diagonal)
      diag_row = max_diagonal < lo ? max_diagonal : lo;               // std::min(lo, max_diagonal)
    }
    // M = Hs + diag / radius: lane i < N holds the row i (its entries j <= i are the ones the factor reads), lane N the
    // right-hand side gs
    double s[N];
    const double damped = Hdiag + diag_row / radius;
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = row == j ? damped : Hrow[j];
    if (lane == N)
    {
#pragma unroll
      for (int j = 0; j < N; ++j) s[j] = gs[j];
    }
    stamp(1);
    // Cholesky and the forward substitution, column by column.  s[jj] of lane i has lost the products of the columns
    // before j, in their order, when column j comes: s[j] of lane j is the pivot's square.  Lu[i][j] = L_ij for
    // j < i < N, Lu[N][j] = y_j, the same value in every lane.
    bool ok = true;
    double rinv[N], Lu[N + 1][N];
#pragma unroll
    for (int j = 0; j < N; ++j)
    {
      const double d = lane_bcast(s[j], j);
      if (!(d > 0.0) || !isfinite(d)) ok = false;
      rinv[j] = 1.0 / __builtin_sqrt(d);
      const double lij = s[j] * rinv[j];
#pragma unroll
      for (int jj = j + 1; jj <= N; ++jj) Lu[jj][j] = lane_bcast(lij, jj);
#pragma unroll
      for (int jj = j + 1; jj < N; ++jj) s[jj] -= lij * Lu[jj][j];
    }
    double y[N];
#pragma unroll
    for (int i = N - 1; i >= 0; --i)
    {
      double t = Lu[N][i];
#pragma unroll
      for (int k = i + 1; k < N; ++k) t -= Lu[k][i] * y[k];
      y[i] = t * rinv[i];
    }
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (!isfinite(y[i])) ok = false;
    stamp(2);
    reuse_diagonal = 1;
    // the model's cost change (meaningless, and not used, when the solve failed)
    double step[N], t_row = 0, sg = 0, sHs = 0;
#pragma unroll
    for (int a = 0; a < N; ++a) step[a] = -y[a];
#pragma unroll
    for (int b = 0; b < N; ++b) t_row += Hrow[b] * step[b];
#pragma unroll
    for (int a = 0; a < N; ++a)
    {
      sg += step[a] * gs[a];
      sHs += step[a] * lane_bcast(t_row, a);
    }
    const double change = -sg - 0.5 * sHs;
    if (!ok || change < 0.0)
    {
      ++unsuccessful;
      if (++consecutive_invalid >= max_consecutive_invalid) { code = kCodeInvalidSteps; break; }
      radius /= decrease_factor; decrease_factor *= 2.0;
      continue;
    }
    consecutive_invalid = 0;
    model_cost_change = change;
    double dn = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a) cand[a] = x[a];
#pragma unroll
    for (int a = 0; a < N; ++a)
    {
      cand[lm_act<N>(a)] = x[lm_act<N>(a)] + step[a] * scale[a];
      const double e = x[lm_act<N>(a)] - cand[lm_act<N>(a)];
      dn += e * e;
    }
    delta_norm = __builtin_sqrt(dn);
    ++evaluations;
    break;
  }

  // ---- the state for the next evaluation, or for the result
  if (lane < N) lm.diag[lane] = diag_row;
  if (l0)
  {
    if (use_tot && !first)
    {
#pragma unroll
      for (int a = 0; a < 6; ++a) lm.x[a] = x[a];
    }
    lm.cur_buf = cur_buf;
    lm.x_norm = x_norm; lm.radius = radius; lm.decrease_factor = decrease_factor;
    lm.model_cost_change = model_cost_change; lm.delta_norm = delta_norm;
    lm.reuse_diagonal = reuse_diagonal; lm.consecutive_invalid = consecutive_invalid;
    lm.iter = iter; lm.iterations = iter;
    lm.successful = successful; lm.unsuccessful = unsuccessful; lm.evaluations = evaluations;
    lm.code = code;
    sh.stop = code != kCodeNone ? 1 : 0;
  }
  stamp(3);
  return code != kCodeNone;
}

// What the host's loop does between two ICP iterations (host/lsa_slam_icp.cpp, Slam.cxx:940-950 / 1134-1151), for the
// iteration enqueued behind this solve: does it run (the solve was not skipped and made a step), the pose from the solve's
// parameters, the next start point (the round trip through the matrix, as LocalOptimizer::SetPosePrior makes it) and,
// localization, Slam::RefineUndistortion under the new pose.  lsa_posemath.h is the host's arithmetic: the host works
// the same values out from the same result when it arrives, bit for bit.  One wavefront: the six half-angle
// cosines / sines side by side, the rest on lane 0.
__device__ void leave_link(const LmParams& p, const LmState& lm, bool failed, int part)
{
  using namespace posemath;
  IcpLinkBlock* g = p.leave;
  const int lane = threadIdx.x & 63;
  const bool go = !failed && !lm.skipped && lm.successful != 1;
  if (!go)
  {
    if (lane == 0 && part == 0) g->go = 0ull;
    return;
  }
  // two wavefronts side by side (the block is read after the kernel has ended: no order among its words): part 0 -- go,
  // pose, start point; part 1 -- the undistortion.  Both work the pose out for themselves (the same bits).
  if (part == 1 && !p.link_refine) return;
  const double half = lm.x[3 + (lane < 6 ? lane % 3 : 0)] * 0.5;
  const double v = lane < 3 ? lsa_cos(half) : lsa_sin(half);
  const double cx = lane_value(v, 0), cy = lane_value(v, 1), cz = lane_value(v, 2);
  const double sx = lane_value(v, 3), sy = lane_value(v, 4), sz = lane_value(v, 5);
  double x[6];
#pragma unroll
  for (int a = 0; a < 6; ++a) x[a] = lm.x[a];
  const Pose T = FromXYZRPYTrig(x, cx, sx, cy, sy, cz, sz);
  if (part == 0)
  {
    if (lane != 0) return;
    double x0[6];
    ToXYZRPY(T, x0);
    g->in.pose = ToRigid(T);
#pragma unroll
    for (int a = 0; a < 6; ++a) g->in.x0[a] = x0[a];
    g->go = 1ull;
    return;
  }
  WithinFrameMotion m;
  double mv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) mv[i] = p.motion0[i];
  if (!p.motion_from_args)
  {
#pragma unroll
    for (int i = 0; i < 16; ++i) mv[i] = p.motion_dev[i];
  }
  m.Time0 = mv[0]; m.Time1 = mv[1];
  m.Rot0 = {mv[2], mv[3], mv[4], mv[5]};
  m.Rot1 = {mv[6], mv[7], mv[8], mv[9]};
#pragma unroll
  for (int i = 0; i < 3; ++i) { m.Trans0[i] = mv[10 + i]; m.Trans1[i] = mv[13 + i]; }
  // Slam::RefineUndistortion with the scan's pose at its begin (lane 0) and at its end (lane 1) interpolated side by
  // side; lane 0 takes the end over and goes on alone
  const Pose previous = FromRigid(p.previous_world);
  const Pose mine = InterpolateScanPose(p.clock, previous, T, lane == 1 ? m.Time1 : m.Time0);
  Pose worldToBaseEnd = Pose::Identity();
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) worldToBaseEnd(i, j) = lane_value(mine(i, j), 1);
  if (lane != 0) return;
  Pose d0, d1;
  RefineUndistortionFrom(m, mine, worldToBaseEnd, T, d0, d1);
  g->in.ic = MakeInterpConst(d0, d1, m.Time0, m.Time1);
  double* o = p.motion_dev;
  o[0] = m.Time0; o[1] = m.Time1;
  o[2] = m.Rot0.w; o[3] = m.Rot0.x; o[4] = m.Rot0.y; o[5] = m.Rot0.z;
  o[6] = m.Rot1.w; o[7] = m.Rot1.x; o[8] = m.Rot1.y; o[9] = m.Rot1.z;
#pragma unroll
  for (int i = 0; i < 3; ++i) { o[10 + i] = m.Trans0[i]; o[13 + i] = m.Trans1[i]; }
}

__global__ __launch_bounds__(kLmThreads) void k_lm_solve(LmParams p, u64* __restrict__ xchg, u64* __restrict__ mailbox, unsigned out_tag, unsigned long long* trace)
{
  __shared__ Shared sh;
  extern __shared__ double lm_cache[];  // [17][cslots * kLmThreads]
  const bool tr = trace != nullptr && blockIdx.x == 0;
  // the thread's first residual block: on its way from memory while the launch finds out whether it runs and where it starts
  RecordRegs pre;
  if (kRecordPrefetch && p.cslots > 0) record_load(p.set, blockIdx.x * blockDim.x + threadIdx.x, pre);
  if (p.link)
  {
    // enqueued ahead of its start point: the solve in front of this launch has left it (go == 1), or the iteration was
    // called off (0: nobody waits for a result)
    if (p.link->go != 1ull)
    {
      // an iteration that does not run leaves the same for the one behind it
      if (p.leave && blockIdx.x == 0 && threadIdx.x == 0) p.leave->go = 0ull;
      return;
    }
  }
  if (threadIdx.x < 64)
  {
    // the start point: the launch's own argument, or what the link brought over (the arguments stay untouched)
    double x0[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) x0[a] = p.x0[a];
    if (p.link)
    {
#pragma unroll
      for (int a = 0; a < 6; ++a) x0[a] = p.link->in.x0[a];
    }
    if (threadIdx.x == 0)
    {
      for (int i = 0; i < 6; ++i) sh.lap[i] = 0;
      for (int i = 0; i < 4; ++i) sh.sub[i] = 0;
      sh.st0 = 0;
      sh.tk = wall_clock64();
      sh.lap[5] = sh.tk;
      // (k_selftest_lm_step starts the step from THE SAME VALUES: the two must stay equal)
      LmState& lm = sh.lm;
#pragma unroll
      for (int v = 0; v < kAccumVals; ++v) sh.sums[0][v] = 0.;
      lm.cur_buf = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) { lm.x[a] = x0[a]; lm.scale[a] = 1.; lm.diag[a] = 0.; }
      lm.radius = 1e4; lm.decrease_factor = 2.0; lm.x_norm = 0.; lm.model_cost_change = 0.; lm.delta_norm = 0.; lm.initial_cost = 0.;
      lm.reuse_diagonal = 0; lm.consecutive_invalid = 0; lm.iter = 0;
      lm.evaluations = 1; lm.successful = 0; lm.unsuccessful = 0; lm.iterations = 0; lm.code = kCodeNone; lm.skipped = 0; lm.matches = 0;
      sh.stop = 0;
    }
    finish_point(sh, x0[0], x0[1], x0[2], x0[3], x0[4], x0[5]);
  }
  if (kRecordPrefetch && p.cslots > 0) record_stash(pre, lm_cache, p.cslots * kLmThreads, threadIdx.x);
  __syncthreads();
  bool failed = false;
  // every evaluation of the launch has an epoch of its own; all blocks walk through the same sequence of them
  for (unsigned epoch = 1;; ++epoch)
  {
    if (!lm_evaluate(p, epoch, xchg, sh, lm_cache, tr)) { failed = true; break; }
    if (threadIdx.x < 64)
    {
      if (threadIdx.x == 0 && tr) sh.st0 = wall_clock64();
      double cand[6];
      const bool stop = p.two_d ? lm_step<3>(p, sh, epoch == 1, cand) : lm_step<6>(p, sh, epoch == 1, cand);
      // the candidate's rotation and derivatives -- unless the solve is over: nobody evaluates at sh.w then, and neither
      // the result nor the link reads sh.w or sh.rot (they take the pose from LmState::x)
      if (!stop) finish_point(sh, cand[0], cand[1], cand[2], cand[3], cand[4], cand[5]);
    }
    __syncthreads();
    if (tr) lm_lap(sh, 3);
    if (sh.stop) break;
  }
  if (blockIdx.x != 0) return;
  if (tr && threadIdx.x == 0)
  {
    for (int i = 0; i < 4; ++i) trace[i] += sh.lap[i];
    trace[4] += (unsigned long long)sh.lm.evaluations;
    trace[5] += wall_clock64() - sh.lap[5];
    trace[6] += 1;
    trace[7] += sh.lap[4];  // of "evaluate": the residual blocks alone (before the wavefront's reduction)
    for (int i = 0; i < 4; ++i) trace[8 + i] += sh.sub[i];
  }
  // the iteration enqueued behind this solve: the second and third wavefronts prepare what it reads while the first sends the result
  if (p.leave && threadIdx.x >= 64 && threadIdx.x < 192) leave_link(p, sh.lm, failed, (threadIdx.x >> 6) - 1);
  // every block holds the same result; block 0's copy goes out as 2 granules per double
  if (threadIdx.x < 2 * kResCount)
  {
    const LmState& lm = sh.lm;
    const int v = threadIdx.x >> 1, half = threadIdx.x & 1;
    double r = 0.;
    if (v < kResInitial) r = lm.x[v - kResPose];
    else if (v == kResInitial) r = lm.initial_cost;
    else if (v == kResFinal) r = sh.sums[lm.cur_buf][0];
    else if (v < kResSums + kAccumVals) r = sh.sums[lm.cur_buf][v - kResSums];
    else if (v == kResSuccessful) r = lm.successful;
    else if (v == kResUnsuccessful) r = lm.unsuccessful;
    else if (v == kResIterations) r = lm.iterations;
    else if (v == kResEvaluations) r = lm.evaluations;
    else if (v == kResSkipped) r = lm.skipped;
    else if (v == kResCode) r = lm.code;
    else if (v == kResMatches) r = lm.matches;
    else if (v == kResFailed) r = failed ? 1. : 0.;
    const u64 bits = (u64)__double_as_longlong(r);
    const unsigned word = half ? (unsigned)(bits >> 32) : (unsigned)(bits & 0xffffffffull);
    __hip_atomic_store(mailbox + threadIdx.x, ((u64)out_tag << 32) | word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// lsa_selftest_lm_step: lm_step on scripted sums, a workgroup of one wavefront per script.  What k_lm_solve's first
// wavefront does between two evaluations, with the evaluation replaced by 29 values read from the script: the fold's last
// store into sh.sums[1 - cur_buf], the step, the candidate's rotation, and one record of the state the step left.
constexpr int kStepRecord = 42;  // include/lidarslam_amd.h: the record of lsa_selftest_lm_step
__global__ __launch_bounds__(64) void k_selftest_lm_step(const int* __restrict__ header, const int* __restrict__ first_eval, const double* __restrict__ x0s,
                                                         const double* __restrict__ sums, double* __restrict__ records, double* __restrict__ results,
                                                         int* __restrict__ status)
{
  __shared__ Shared sh;
  const int s = blockIdx.x;
  const int two_d = header[4 * s], evals = header[4 * s + 3];
  const size_t first = (size_t)first_eval[s];
  LmParams p;  // (lm_step reads max_iter and min_matches, nothing else)
  p.max_iter = header[4 * s + 1];
  p.min_matches = header[4 * s + 2];
  {
    double x0[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) x0[a] = x0s[(size_t)s * 6 + a];
    if (threadIdx.x == 0)
    {
      // THE SAME VALUES as the head of k_lm_solve: the two must stay equal (st0 = 0: the step traces nothing)
      for (int i = 0; i < 6; ++i) sh.lap[i] = 0;
      for (int i = 0; i < 4; ++i) sh.sub[i] = 0;
      sh.st0 = 0;
      sh.tk = 0;
      LmState& lm = sh.lm;
#pragma unroll
      for (int v = 0; v < kAccumVals; ++v) sh.sums[0][v] = 0.;
      lm.cur_buf = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) { lm.x[a] = x0[a]; lm.scale[a] = 1.; lm.diag[a] = 0.; }
      lm.radius = 1e4; lm.decrease_factor = 2.0; lm.x_norm = 0.; lm.model_cost_change = 0.; lm.delta_norm = 0.; lm.initial_cost = 0.;
      lm.reuse_diagonal = 0; lm.consecutive_invalid = 0; lm.iter = 0;
      lm.evaluations = 1; lm.successful = 0; lm.unsuccessful = 0; lm.iterations = 0; lm.code = kCodeNone; lm.skipped = 0; lm.matches = 0;
      sh.stop = 0;
      sh.failed = 0;
    }
    finish_point(sh, x0[0], x0[1], x0[2], x0[3], x0[4], x0[5]);
  }
  __syncthreads();
  int used = 0;
  bool stopped = false;
  while (used < evals && !stopped)
  {
    // as the last lines of lm_evaluate's fold: lane v stores value v of the evaluation, the step's loads follow in order
    if (threadIdx.x < kAccumVals) sh.sums[1 - sh.lm.cur_buf][threadIdx.x] = sums[(first + used) * kAccumVals + threadIdx.x];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    double cand[6];
    const bool stop = two_d ? lm_step<3>(p, sh, used == 0, cand) : lm_step<6>(p, sh, used == 0, cand);
    if (!stop) finish_point(sh, cand[0], cand[1], cand[2], cand[3], cand[4], cand[5]);
    __syncthreads();
    if (threadIdx.x == 0)
    {
      const LmState& lm = sh.lm;
      double* o = records + (first + used) * kStepRecord;
#pragma unroll
      for (int a = 0; a < 6; ++a) o[a] = stop ? 0. : cand[a];
      o[6] = lm.code; o[7] = sh.stop;
      o[8] = lm.radius; o[9] = lm.decrease_factor; o[10] = lm.x_norm; o[11] = lm.model_cost_change; o[12] = lm.delta_norm; o[13] = lm.initial_cost;
      o[14] = lm.reuse_diagonal; o[15] = lm.consecutive_invalid; o[16] = lm.iter; o[17] = lm.evaluations; o[18] = lm.successful;
      o[19] = lm.unsuccessful; o[20] = lm.iterations; o[21] = lm.skipped; o[22] = lm.matches;
      for (int a = 0; a < 6; ++a) { o[23 + a] = lm.x[a]; o[29 + a] = lm.scale[a]; o[35 + a] = lm.diag[a]; }
      o[41] = lm.cur_buf;
    }
    ++used;
    stopped = sh.stop != 0;
    __syncthreads();
  }
  if (threadIdx.x == 0) { status[2 * s] = stopped ? 0 : 1; status[2 * s + 1] = used; }
  // the result as k_lm_solve composes it: the pose and the counts from LmState, the sums from the buffer cur_buf names
  if (threadIdx.x < kResCount)
  {
    const LmState& lm = sh.lm;
    const int v = threadIdx.x;
    double r = 0.;
    if (v < kResInitial) r = lm.x[v - kResPose];
    else if (v == kResInitial) r = lm.initial_cost;
    else if (v == kResFinal) r = sh.sums[lm.cur_buf][0];
    else if (v < kResSums + kAccumVals) r = sh.sums[lm.cur_buf][v - kResSums];
    else if (v == kResSuccessful) r = lm.successful;
    else if (v == kResUnsuccessful) r = lm.unsuccessful;
    else if (v == kResIterations) r = lm.iterations;
    else if (v == kResEvaluations) r = lm.evaluations;
    else if (v == kResSkipped) r = lm.skipped;
    else if (v == kResCode) r = lm.code;
    else if (v == kResMatches) r = lm.matches;
    results[(size_t)s * kResCount + v] = stopped ? r : 0.;  // (a script that ran out has no result)
  }
}

const char* const kMessages[] = {"", "not enough matches", "gradient tolerance (iteration 0)", "max iterations", "gradient tolerance",
                                 "min trust region radius", "too many invalid steps", "parameter tolerance", "function tolerance"};

}  // namespace

namespace lsa
{
std::atomic<int> g_live_contexts{0};
// workgroups one solve may use so that the solves that can run at once all fit on the chip
int lm_blocks_share()
{
  static const int cus = [] {
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
    return std::max(prop.multiProcessorCount, 8);
  }();
  static const int queues = [] {
    const char* e = std::getenv("GPU_MAX_HW_QUEUES");
    const int q = e ? std::atoi(e) : 4;  // the runtime's default
    return std::max(q, 1);
  }();
  const int side_by_side = std::max(1, std::min(g_live_contexts.load(std::memory_order_relaxed), queues));
  return std::max(cus / side_by_side, 8);
}
// how many layers of residual blocks (a layer: one block per thread, 17 * kLmThreads doubles = 68 KiB) the solve kernel
// may keep in LDS beside its own static data (Shared, 3 360 B).  A layer is counted only when the runtime accepts it as
// dynamic LDS AND static + dynamic fit the LDS a workgroup may have (160 KiB on gfx950: two layers, since the fold no
// longer keeps the granules in LDS): whether the runtime's check counts the static part is not something to rely on.
int lm_cache_capacity()
{
  const size_t layer = (size_t)17 * kLmThreads * sizeof(double);
  size_t limit = 0, static_bytes = 0;
  {
    hipDeviceProp_t prop;
    int dev = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) limit = std::max(prop.sharedMemPerBlock, (size_t)prop.maxSharedMemoryPerMultiProcessor);
    hipFuncAttributes attr;
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(k_lm_solve)) == hipSuccess) static_bytes = attr.sharedSizeBytes;
  }
  int slots = 0;
  for (int want = 3; want >= 1 && slots == 0; --want)
    if ((limit == 0 || static_bytes + want * layer <= limit) &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(k_lm_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(want * layer)) == hipSuccess)
      slots = want;
  (void)hipGetLastError();
  return slots;
}
}  // namespace lsa

extern "C" {

static int solve_device_begin(lsa_ctx* ctx, unsigned type_mask, const double prior[6], int two_d_mode, int lm_max_iter, int min_matches, int leave_ticket, const lsa_icp_link_t* link)
{
  if (!ctx) return LSA_E_ARG;
  if (leave_ticket >= 0 && (leave_ticket >= kLinkRing || !link || !ctx->link_dev || !ctx->link_saved[leave_ticket].used))
    return ctx->fail(LSA_E_ARG, "lsa_solve_device_begin_linked: no such link (lsa_icp_link)");
  if (!prior && ctx->link_current < 0) return ctx->fail(LSA_E_ARG, "lsa_solve_device_begin: no start point and no link to wait behind");
  if (!ctx->lm_mailbox) return ctx->fail(LSA_E_STATE, "lsa_solve_device: no coherent host memory for the result");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LmParams p;
  int total = 0;
  for (int k = 0; k < 3; ++k)
  {
    MatchBuf& mb = ctx->match[k];
    const bool use = (type_mask >> k) & 1u && mb.valid && mb.k > 0;
    p.set.rec[k] = mb.rec; p.set.status[k] = mb.status; p.set.cap[k] = mb.cap;
    p.set.count[k] = use ? mb.k : 0;
    p.set.sat2[k] = mb.sat * mb.sat;
    total += p.set.count[k];
  }
  for (int a = 0; a < 6; ++a) p.x0[a] = prior ? prior[a] : 0.;
  p.give_up_block = ctx->debug_lm_give_up_block;
  ctx->debug_lm_give_up_block = -1;
  p.link = prior ? nullptr : reinterpret_cast<const IcpLinkBlock*>(ctx->link_dev + (size_t)ctx->link_current * kLinkWords);
  p.leave = nullptr;
  p.link_refine = 0;
  p.motion_from_args = 0;
  p.motion_dev = ctx->motion_dev;
  std::memset(&p.clock, 0, sizeof(p.clock));
  std::memset(&p.previous_world, 0, sizeof(p.previous_world));
  std::memset(p.motion0, 0, sizeof(p.motion0));
  if (leave_ticket >= 0)
  {
    p.leave = reinterpret_cast<IcpLinkBlock*>(ctx->link_dev + (size_t)leave_ticket * kLinkWords);
    p.link_refine = link->refine_undistortion ? 1 : 0;
    p.motion_from_args = link->first ? 1 : 0;
    p.clock.have_log = link->have_log ? 1 : 0;
    p.clock.prev_time = link->prev_time;
    p.clock.cur_time = link->cur_time;
    p.clock.max_ratio = link->max_extrapolation_ratio;
    row_major_to_rt(link->previous_world, p.previous_world.R, p.previous_world.t);
    std::memcpy(p.motion0, link->motion, sizeof(p.motion0));
  }
  p.sensors = ctx->sensor_terms;
  p.sensors_on = (ctx->sensor_terms.wheel || ctx->sensor_terms.gravity) ? 1 : 0;
  p.two_d = two_d_mode ? 1 : 0;
  p.max_iter = lm_max_iter < 0 ? 0 : lm_max_iter;
  p.min_matches = min_matches;
  // every evaluation of the launch takes a tag of its own; tags of earlier launches never come back within 2^32
  p.tag_base = ctx->lm_tag;
  ctx->lm_tag += (unsigned)p.max_iter + 4u;
  const unsigned out_tag = (unsigned)(++ctx->lm_seq);
  // about two residual blocks per thread (measured: 1024 per workgroup 63 us a solve, 512: 56, 256: 58 -- fewer blocks per thread
  // shorten the evaluation, more workgroups lengthen the exchange), never more workgroups than the exchange has slots for
  // ... and never more than this solve's share of the chip: the workgroups exchange their sums by waiting for each other,
  // so ALL of them have to be resident (512 threads of 250 registers: one workgroup per CU), also when the solves of
  // other contexts of this process run beside this one -- as many at once as the process has hardware queues
  const int nb = std::min(std::max((total + ctx->lm_records - 1) / ctx->lm_records, 1), std::min(std::min(ctx->lm_blocks, kLmBlocksMax), lm_blocks_share()));
  // the thread's first residual blocks stay in LDS between the evaluations (17 doubles each): as many per thread as
  // the block's share needs, as many as the LDS holds beside the kernel's own 3 KB (the rest is read again)
  const int per_thread = (total + nb * kLmThreads - 1) / (nb * kLmThreads);
  const size_t slot_bytes = (size_t)17 * kLmThreads * sizeof(double);
  p.cslots = std::min(per_thread, std::max(ctx->lm_cache_slots, 0));
  ctx->lm_shape[0] = nb; ctx->lm_shape[1] = per_thread; ctx->lm_shape[2] = p.cslots; ctx->lm_shape[3] = total;
  {
    ProfScope ps(ctx, "lm_solve", 0.);
    hipLaunchKernelGGL(k_lm_solve, dim3(nb), dim3(kLmThreads), p.cslots * slot_bytes, ctx->stream, p, ctx->lm_xchg, ctx->lm_mailbox + (size_t)(out_tag % kLmMailRing) * 2 * kLmOut, out_tag,
                       ctx->route_stats && ctx->trace_dev ? reinterpret_cast<unsigned long long*>(ctx->trace_dev) + (size_t)8192 * 12 : nullptr);
  }
  ctx->lm_pending.push_back(out_tag);
  ctx->lm_pending_wait.push_back(prior ? -1 : ctx->link_current);
  // what is enqueued next waits behind the link this solve leaves
  if (leave_ticket >= 0) ctx->link_current = leave_ticket;
  if (lsa_icp_trace_on()) std::fprintf(stderr, "[lm begin] tag %u linked %d leaves %d sat2 %.6g %.6g counts %d %d\n", out_tag, prior ? 0 : 1, leave_ticket, p.set.sat2[0], p.set.sat2[1], p.set.count[0], p.set.count[1]);
  return LSA_OK;
}

int lsa_solve_device_begin(lsa_ctx* ctx, unsigned type_mask, const double prior[6], int two_d_mode, int lm_max_iter, int min_matches)
{
  return solve_device_begin(ctx, type_mask, prior, two_d_mode, lm_max_iter, min_matches, -1, nullptr);
}

int lsa_solve_device_begin_linked(lsa_ctx* ctx, unsigned type_mask, const double prior[6], int two_d_mode, int lm_max_iter, int min_matches, int leave_ticket, const lsa_icp_link_t* link)
{
  if (ctx && (int)ctx->lm_pending.size() >= kLmMailRing - 1) return ctx->fail(LSA_E_STATE, "lsa_solve_device_begin_linked: too many solves in flight");
  return solve_device_begin(ctx, type_mask, prior, two_d_mode, lm_max_iter, min_matches, leave_ticket, link);
}

int lsa_solve_device_drop(lsa_ctx* ctx)
{
  if (!ctx || ctx->lm_pending.empty()) return LSA_E_ARG;
  ctx->lm_pending.pop_back();  // the solve begun last will never run (its link was called off): nobody waits for it
  ctx->lm_pending_wait.pop_back();
  return LSA_OK;
}

int lsa_solve_device_end(lsa_ctx* ctx, lsa_solve_result_t* out)
{
  if (!ctx || !out) return ctx ? ctx->fail(LSA_E_ARG, "lsa_solve_device_end: bad argument") : LSA_E_ARG;
  if (ctx->lm_pending.empty()) return ctx->fail(LSA_E_STATE, "lsa_solve_device_end: no solve in flight");
  const unsigned out_tag = ctx->lm_pending.front();
  ctx->lm_pending.pop_front();
  const int waited_behind = ctx->lm_pending_wait.front();
  ctx->lm_pending_wait.pop_front();
  if (lsa_icp_trace_on()) std::fprintf(stderr, "[lm end] waits for tag %u (%zu more in flight)\n", out_tag, ctx->lm_pending.size());
  // the result arrives as granules in coherent host memory (as lsa_accumulate's sums do)
  double res[kResCount];
  const unsigned long long* box = ctx->lm_mailbox + (size_t)(out_tag % kLmMailRing) * 2 * kLmOut;  // (solves in flight do not share a mailbox)
  {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (int v = 0; v < kResCount; ++v)
    {
      unsigned long long g[2];
      for (int h = 0; h < 2; ++h)
        while (((g[h] = __atomic_load_n(box + 2 * v + h, __ATOMIC_RELAXED)) >> 32) != out_tag)
        {
          if ((++spins & 0x3ff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2000))
          {
            // whatever was enqueued ahead is called off first: what its matches announced on the host -- the NEXT
            // iteration's saturation distance -- must not be what the caller's fall-back solves with
            (void)lsa_icp_abandon(ctx);
            LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
            return ctx->fail(LSA_E_STATE, "lsa_solve_device: no result from the device");
          }
#if defined(__x86_64__)
          __builtin_ia32_pause();
#endif
        }
      const unsigned long long bits = ((g[1] & 0xffffffffull) << 32) | (g[0] & 0xffffffffull);
      std::memcpy(&res[v], &bits, sizeof(double));
    }
  }
  if (lsa_icp_trace_on()) std::fprintf(stderr, "[lm end] tag %u: failed %g code %g evals %g matches %g\n", out_tag, res[kResFailed], res[kResCode], res[kResEvaluations], res[kResMatches]);
  if (res[kResFailed] != 0.)
  {
    // iterations enqueued ahead are called off first
    (void)lsa_icp_abandon(ctx);
    LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // every block has given up or finished: the slots are quiet again
    ctx->lm_fallbacks++;
    return ctx->fail(LSA_E_STATE, "lsa_solve_device: a block waited too long for the others");
  }
  // the link this solve waited behind has served: its iteration ran, what its match announced stands
  if (waited_behind >= 0 && waited_behind < kLinkRing) ctx->link_saved[waited_behind].used = false;
  std::memset(out, 0, sizeof(*out));
  for (int a = 0; a < 6; ++a) out->pose[a] = res[kResPose + a];
  out->initial_cost = res[kResInitial];
  out->final_cost = res[kResFinal];
  out->cost = res[kResSums];
  for (int a = 0; a < 6; ++a) out->g[a] = res[kResSums + 1 + a];
  {
    int h = kResSums + 7;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) { out->H[a * 6 + b] = res[h]; out->H[b * 6 + a] = res[h]; ++h; }
  }
  out->num_successful_steps = (int)res[kResSuccessful];
  out->num_unsuccessful_steps = (int)res[kResUnsuccessful];
  out->num_iterations = (int)res[kResIterations];
  out->num_evaluations = (int)res[kResEvaluations];
  out->skipped = (int)res[kResSkipped];
  out->termination = (int)res[kResCode];
  out->num_matches = (int)res[kResMatches];
  out->message = kMessages[std::min(std::max(out->termination, 0), 8)];
  // algorithmic bytes: every evaluation reads the record of every residual block (128 B + status)
  profile_add_bytes(ctx, "lm_solve", (double)out->num_evaluations * out->num_matches * 129);
  return LSA_OK;
}

int lsa_solve_device(lsa_ctx* ctx, unsigned type_mask, const double prior[6], int two_d_mode, int lm_max_iter, int min_matches, lsa_solve_result_t* out)
{
  if (!ctx || !prior || !out) return ctx ? ctx->fail(LSA_E_ARG, "lsa_solve_device: bad argument") : LSA_E_ARG;
  if (!ctx->lm_pending.empty()) return ctx->fail(LSA_E_STATE, "lsa_solve_device: another solve is in flight (lsa_solve_device_begin)");
  const int rc = lsa_solve_device_begin(ctx, type_mask, prior, two_d_mode, lm_max_iter, min_matches);
  if (rc) return rc;
  // host work the caller wants done while the kernel runs (one shot)
  if (ctx->solve_hook)
  {
    void (*fn)(void*) = ctx->solve_hook;
    ctx->solve_hook = nullptr;
    fn(ctx->solve_hook_arg);
  }
  return lsa_solve_device_end(ctx, out);
}

// ---- ICP iterations enqueued ahead of their inputs ------------------------------------------------------------------
// A link is a block on the device that carries what the launches of the next iteration need (the pose the solve before it
// ended with: slam_lib/src/Slam.cxx:907, 940-946 and 1086, 1134-1142), or calls them off.  It is written by the SOLVE in
// front of it (k_lm_solve's leave_link: lsa_posemath.h's arithmetic, which the host repeats on the same result when it
// arrives), so that between two iterations there is one kernel boundary -- no kernel-launch path (a dozen microseconds a
// launch), no trip over the bus, no host thread on the path.  The ticket is
// reserved here, handed to lsa_solve_device_begin_linked as the block to leave, and what is enqueued after that solve
// (lsa_match_types_linked, the next solve) waits behind it.
int lsa_icp_link(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  if (!ctx->link_dev || !ctx->motion_dev) return ctx->fail(LSA_E_STATE, "lsa_icp_link: no device memory for the links");
  const unsigned seq = ctx->link_seq + 1;
  const int ticket = (int)(seq % kLinkRing);
  if (ctx->link_saved[ticket].used) return ctx->fail(LSA_E_STATE, "lsa_icp_link: too many iterations enqueued ahead");
  ctx->link_seq = seq;
  lsa_ctx::LinkSaved& sv = ctx->link_saved[ticket];
  sv = lsa_ctx::LinkSaved();
  sv.used = true;
  sv.seq = seq;
  return ticket;
}

// What the HOST works out between two iterations from a solve's result (lsa_posemath.h compiled for this side: the loops
// of host/lsa_slam_icp.cpp call the same functions), laid out as the device's block: a test holds lsa_icp_link_peek
// against it, word for word.
int lsa_icp_link_expected(const double x[6], int skipped, int successful_steps, const lsa_icp_link_t* link, unsigned long long words[64], double motion_after[16])
{
  if (!x || !link || !words) return LSA_E_ARG;
  using namespace posemath;
  IcpLinkBlock g;
  std::memset(&g, 0, sizeof(g));
  std::memset(words, 0, kLinkWords * sizeof(unsigned long long));
  if (motion_after) std::memcpy(motion_after, link->motion, 16 * sizeof(double));
  if (skipped || successful_steps == 1) return LSA_OK;  // go = 0: nothing else of the block means anything
  const Pose T = FromXYZRPY(x);
  ToXYZRPY(T, g.in.x0);
  g.in.pose = ToRigid(T);
  if (link->refine_undistortion)
  {
    WithinFrameMotion m;
    const double* mv = link->motion;
    m.Time0 = mv[0]; m.Time1 = mv[1];
    m.Rot0 = {mv[2], mv[3], mv[4], mv[5]};
    m.Rot1 = {mv[6], mv[7], mv[8], mv[9]};
    for (int i = 0; i < 3; ++i) { m.Trans0[i] = mv[10 + i]; m.Trans1[i] = mv[13 + i]; }
    ScanPoseClock clock;
    clock.have_log = link->have_log ? 1 : 0;
    clock.prev_time = link->prev_time;
    clock.cur_time = link->cur_time;
    clock.max_ratio = link->max_extrapolation_ratio;
    Pose previous, d0, d1;
    std::memcpy(previous.m, link->previous_world, sizeof(previous.m));
    // (the device keeps R and t of PreviousTworld: the last row is (0, 0, 0, 1) by construction)
    previous = FromRigid(ToRigid(previous));
    RefineUndistortion(m, clock, previous, T, d0, d1);
    g.in.ic = MakeInterpConst(d0, d1, m.Time0, m.Time1);
    if (motion_after)
    {
      double* o = motion_after;
      o[0] = m.Time0; o[1] = m.Time1;
      o[2] = m.Rot0.w; o[3] = m.Rot0.x; o[4] = m.Rot0.y; o[5] = m.Rot0.z;
      o[6] = m.Rot1.w; o[7] = m.Rot1.x; o[8] = m.Rot1.y; o[9] = m.Rot1.z;
      for (int i = 0; i < 3; ++i) { o[10 + i] = m.Trans0[i]; o[13 + i] = m.Trans1[i]; }
    }
  }
  g.go = 1ull;
  std::memcpy(words, &g, sizeof(g));
  return LSA_OK;
}

int lsa_icp_link_peek(lsa_ctx* ctx, int ticket, unsigned long long words[64])
{
  if (!ctx || !words || ticket < 0 || ticket >= kLinkRing || !ctx->link_dev) return ctx ? ctx->fail(LSA_E_ARG, "lsa_icp_link_peek: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LSA_HIP(ctx, hipMemcpy(words, ctx->link_dev + (size_t)ticket * kLinkWords, kLinkWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return LSA_OK;
}

int lsa_icp_cancel(lsa_ctx* ctx, int ticket)
{
  if (!ctx || ticket < 0 || ticket >= kLinkRing) return LSA_E_ARG;
  // what the launches behind the link had announced on the host is taken back: they will not run
  // (the device has called it off itself -- the solve in front left go = 0 -- or will never reach it)
  const lsa_ctx::LinkSaved sv = ctx->link_saved[ticket];
  if (!sv.used) return ctx->fail(LSA_E_ARG, "lsa_icp_cancel: no such link");
  ctx->link_saved[ticket].used = false;
  if (ctx->link_current == ticket) ctx->link_current = -1;
  for (int k = 0; k < 3; ++k)
    if ((sv.mask >> k) & 1u)
    {
      ctx->match[k].sat = sv.sat[k];
      ctx->match[k].k = sv.k[k];
      ctx->match[k].valid = sv.valid[k];
      ctx->hist_pos[k] = sv.hist_pos[k];
      ctx->hist_serial[k] = sv.hist_serial[k];
    }
  return LSA_OK;
}

int lsa_icp_abandon(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  // the youngest first: each takes back what ITS match announced, the oldest one's "before" is what remains
  while (true)
  {
    int youngest = -1;
    for (int t = 0; t < kLinkRing; ++t)
      if (ctx->link_saved[t].used && (youngest < 0 || (int)(ctx->link_saved[t].seq - ctx->link_saved[youngest].seq) > 0)) youngest = t;
    if (youngest < 0) break;
    if (lsa_icp_cancel(ctx, youngest) != LSA_OK) ctx->link_saved[youngest].used = false;
  }
  ctx->lm_pending.clear();
  ctx->lm_pending_wait.clear();
  ctx->link_current = -1;
  return LSA_OK;
}

int lsa_debug_set(lsa_ctx* ctx, const char* name, int value)
{
  if (!ctx || !name) return LSA_E_ARG;
  const std::string n(name);
  const lsa_ctx::ShapeKnobs& c = ctx->created_knobs;
  // the launch-shape knobs: the clamps of the environment variables read at creation (lsa_ctx.hip); negative restores
  if (n == "lm_give_up_block") ctx->debug_lm_give_up_block = value;
  else if (n == "lm_blocks") ctx->lm_blocks = value < 0 ? c.lm_blocks : std::min(std::max(value, 1), kLmBlocksMax);
  else if (n == "lm_records") ctx->lm_records = value < 0 ? c.lm_records : std::min(std::max(value, 256), 4096);
  else if (n == "lm_cache") ctx->lm_cache_slots = value < 0 ? c.lm_cache_slots : std::min(value, ctx->lm_cache_capacity);
  else if (n == "accum_blocks") ctx->accum_blocks = value < 0 ? c.accum_blocks : std::min(std::max(value, 1), kAccumBlocksMax);
  else if (n == "mailbox_check") ctx->mailbox_check = value < 0 ? c.mailbox_check : value != 0;
  else if (n == "pcd_lds") ctx->pcd_lds = value < 0 ? -1 : (value != 0);  // lsa_pcd.hip: the form of the two conversion kernels
  else if (n == "kplog_chunk_kib") ctx->kplog_chunk_bytes = value < 0 ? ((size_t)32 << 20) : (size_t)std::max(value, 1) << 10;  // lsa_kplog.hip: chunks made from now on
  else if (n == "kplog_fail_alloc") ctx->debug_kplog_fail_alloc = value > 0 ? 1 : 0;
  else if (n == "place_max_blocks") ctx->place_max_blocks = value > 0 ? value : 0;  // lsa_place_search.hip: workgroups (k_place_search) or pieces (k_place_search_rows) of a search launch
  else if (n == "place_untiled") ctx->place_untiled = value != 0;  // lsa_place_search.hip: the search's columns one at a time
  else if (n == "place_table_bytes") ctx->place_table_bytes = value > 0 ? value : 0;  // lsa_place_detect.hip: the table's byte budget
  else if (n == "map_describe_slice") ctx->map_describe_slice = value > 0 ? value : 0;  // lsa_map_place.hip: points a slice (the next description's)
  else if (n == "map_describe_cull") ctx->map_describe_cull = value != 0;
  else return ctx->fail(LSA_E_ARG, "lsa_debug_set: no such knob");
  return LSA_OK;
}

int lsa_solve_device_shape(const lsa_ctx* ctx, int out[4])
{
  if (!ctx || !out) return LSA_E_ARG;
  std::memcpy(out, ctx->lm_shape, sizeof(ctx->lm_shape));
  return LSA_OK;
}

int lsa_accumulate_shape(const lsa_ctx* ctx, int out[4])
{
  if (!ctx || !out) return LSA_E_ARG;
  std::memcpy(out, ctx->accum_shape, sizeof(ctx->accum_shape));
  return LSA_OK;
}

int lsa_solve_device_fallbacks(const lsa_ctx* ctx) { return ctx ? ctx->lm_fallbacks : 0; }

int lsa_set_sensor_terms(lsa_ctx* ctx, const lsa_sensor_terms_t* terms)
{
  if (!ctx) return LSA_E_ARG;
  if (terms) ctx->sensor_terms = *terms;
  else std::memset(&ctx->sensor_terms, 0, sizeof(ctx->sensor_terms));
  return LSA_OK;
}

int lsa_solve_device_interlude(lsa_ctx* ctx, void (*fn)(void*), void* arg)
{
  if (!ctx) return LSA_E_ARG;
  ctx->solve_hook = fn;
  ctx->solve_hook_arg = arg;
  return LSA_OK;
}

int lsa_selftest_lm_step(lsa_ctx* ctx, int n_scripts, const int* header, const double* x0, const double* sums, double* records, double* results, int* status)
{
  if (!ctx) return LSA_E_ARG;
  if (n_scripts <= 0 || n_scripts > 65536 || !header || !x0 || !sums || !records || !results || !status) return ctx->fail(LSA_E_ARG, "lsa_selftest_lm_step: bad argument");
  std::vector<int> first(n_scripts);
  size_t total = 0;
  for (int s = 0; s < n_scripts; ++s)
  {
    if (header[4 * s + 1] < 0 || header[4 * s + 3] < 1 || header[4 * s + 3] > 4096) return ctx->fail(LSA_E_ARG, "lsa_selftest_lm_step: a script needs max_iter >= 0 and 1 to 4096 evaluations");
    first[s] = (int)total;
    total += (size_t)header[4 * s + 3];
  }
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  // doubles first (x0, sums, records, results), then the ints (header, first evaluation, status)
  const size_t n = (size_t)n_scripts;
  const size_t doubles = n * 6 + total * kAccumVals + total * kStepRecord + n * kResCount, ints = n * 4 + n + n * 2;
  const int rc = ensure_scratch(ctx, doubles * sizeof(double) + ints * sizeof(int));
  if (rc) return rc;
  double* d_x0 = (double*)ctx->scratch_out;
  double* d_sums = d_x0 + n * 6;
  double* d_records = d_sums + total * kAccumVals;
  double* d_results = d_records + total * kStepRecord;
  int* d_header = (int*)(d_results + n * kResCount);
  int* d_first = d_header + n * 4;
  int* d_status = d_first + n;
  LSA_HIP(ctx, hipMemcpyAsync(d_x0, x0, n * 6 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(d_sums, sums, total * kAccumVals * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(d_header, header, n * 4 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(d_first, first.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipMemsetAsync(d_records, 0, total * kStepRecord * sizeof(double), ctx->stream));  // evaluations behind the stop: zeros
  hipLaunchKernelGGL(k_selftest_lm_step, dim3(n_scripts), dim3(64), 0, ctx->stream, d_header, d_first, d_x0, d_sums, d_records, d_results, d_status);
  LSA_HIP(ctx, hipGetLastError());
  LSA_HIP(ctx, hipMemcpyAsync(records, d_records, total * kStepRecord * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(results, d_results, n * kResCount * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(status, d_status, n * 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

int lsa_solve_device_trace(lsa_ctx* ctx, unsigned long long out[12])
{
  if (!ctx || !out || !ctx->trace_dev) return LSA_E_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return LSA_E_HIP;
  if (hipMemcpy(out, reinterpret_cast<unsigned long long*>(ctx->trace_dev) + (size_t)8192 * 12, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return LSA_E_HIP;
  return LSA_OK;
}

}  // extern "C"
