// lsa_accumulate.hip -- one evaluation of the residual blocks per launch, for the host-driven trust region
// (lsa_solve's fallback loop) and lsa_accumulate: what Ceres evaluates per LM step
// (slam_lib/include/LidarSlam/CeresCostFunctions.h:105-152 + TukeyLoss/ScaledLoss, KeypointsMatcher.cxx:84-101): cost,
// g = J^T r, H = J^T J with a fixed-order wavefront + block + grid reduction (bitwise reproducible run to run).
// The evaluation itself is lsa_accum.h, shared with the device-resident solve of lsa_lm.hip.
#include <chrono>
#include <cmath>
#include "lsa_ctx.h"
#include "lsa_device_math.h"
#include "lsa_accum.h"
#include "lsa_sensor_terms.h"

using namespace lsa;

namespace
{

// One evaluation of the residual blocks (lsa_accum.h) per launch: the host-driven trust region (lsa_accumulate).
__global__ __launch_bounds__(256) void k_accumulate(AccumConst c, double* __restrict__ partials, unsigned long long* __restrict__ mailbox, unsigned tag)
{
  double acc[kAccumVals];
#pragma unroll
  for (int v = 0; v < kAccumVals; ++v) acc[v] = 0.;
  accumulate_records(c.set, c.rot, c.jac != 0, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, acc);
  // fixed-order reduction: wavefront (transposed: permlane swaps + DPP, lsa_accum.h), then the 4 waves through LDS
  __shared__ double wsum[4][kAccumVals];
  int slot;
  const double total = wave_reduce_accum(acc, slot);  // this lane's one value of the 29, summed over the wavefront
  if ((threadIdx.x & 1) == 0 && slot < kAccumVals) wsum[threadIdx.x >> 6][slot] = total;
  __syncthreads();
  // Zero-copy hand-over: the block's 29 partial sums land in coherent host memory as 58 granules.  A granule is
  // ONE naturally aligned 8-byte word -- the evaluation's tag above, one half of a double below -- written by ONE
  // relaxed system-scope atomic store: tag and payload are the same memory object, so the payload can never be
  // seen without its tag, whatever order the fabric delivers the lanes' stores in.  The host polls the granules
  // (relaxed 64-bit atomic loads) and folds the blocks in index order (as k_accumulate_final does): no fence, no
  // flag, no second kernel, no D2H copy, no stream synchronisation on the LM critical path.
  if (threadIdx.x < 2 * kAccumVals)
  {
    const int v = threadIdx.x >> 1, half = threadIdx.x & 1;
    const double r = ((wsum[0][v] + wsum[1][v]) + wsum[2][v]) + wsum[3][v];
    if (half == 0) partials[(size_t)blockIdx.x * kAccumVals + v] = r;
    if (mailbox)
    {
      const unsigned long long bits = (unsigned long long)__double_as_longlong(r);
      const unsigned word = half ? (unsigned)(bits >> 32) : (unsigned)(bits & 0xffffffffull);
      __hip_atomic_store(mailbox + (size_t)blockIdx.x * kMailboxStride + threadIdx.x, ((unsigned long long)tag << 32) | word, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// folds the per-block partials in block order (the path without a mailbox; same order as the host fold)
__global__ void k_accumulate_final(const double* __restrict__ partials, int nblocks, double* __restrict__ out)
{
  const int v = threadIdx.x;
  if (v >= kAccumVals) return;
  double s = 0.;
  for (int b = 0; b < nblocks; ++b) s += partials[(size_t)b * kAccumVals + v];
  out[v] = s;
}

}  // namespace

extern "C" {

int lsa_mailbox_active(const lsa_ctx* ctx) { return ctx && ctx->mailbox ? 1 : 0; }

int lsa_accumulate(lsa_ctx* ctx, unsigned type_mask, const double w[6], int want_jacobian, double* cost, double g[6], double H[36], int* n_valid)
{
  if (!ctx || !w || !cost) return ctx ? ctx->fail(LSA_E_ARG, "lsa_accumulate: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  AccumConst c;
  // R = Rz Ry Rx and its partial derivatives (CeresCostFunctions.h:67-79), once per evaluation on the host
  rotation_and_derivatives(lsa_cos(w[3]), lsa_sin(w[3]), lsa_cos(w[4]), lsa_sin(w[4]), lsa_cos(w[5]), lsa_sin(w[5]), c.rot.R, c.rot.dRx, c.rot.dRy, c.rot.dRz);
  c.rot.t[0] = w[0]; c.rot.t[1] = w[1]; c.rot.t[2] = w[2];
  int total = 0;
  for (int k = 0; k < 3; ++k)
  {
    MatchBuf& mb = ctx->match[k];
    const bool use = (type_mask >> k) & 1u && mb.valid && mb.k > 0;
    c.set.rec[k] = mb.rec; c.set.status[k] = mb.status; c.set.cap[k] = mb.cap;
    c.set.count[k] = use ? mb.k : 0;
    c.set.sat2[k] = mb.sat * mb.sat;
    total += c.set.count[k];
  }
  c.jac = want_jacobian;
  ctx->accum_shape[0] = ctx->accum_blocks;
  ctx->accum_shape[1] = (total + ctx->accum_blocks * 256 - 1) / (ctx->accum_blocks * 256);
  ctx->accum_shape[2] = 0;
  ctx->accum_shape[3] = total;
  hipStream_t st = ctx->stream;
  const unsigned want = (unsigned)(++ctx->mailbox_seq);
  {
    ProfScope ps(ctx, want_jacobian ? "accumulate_jac" : "accumulate_cost", (double)total * 129);
    hipLaunchKernelGGL(k_accumulate, dim3(ctx->accum_blocks), dim3(256), 0, st, c, ctx->partials, ctx->mailbox, want);
  }
  double* hp = ctx->host_pinned + 64;
  bool got = false;
  if (ctx->mailbox)
  {
    // poll the granules (bounded: fall back to a device fold + synchronous copy if one does not arrive); the blocks
    // are folded in index order as they come in
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    bool timeout = false;
    for (int v = 0; v < kAccumVals; ++v) hp[v] = 0.;
    for (int b = 0; b < ctx->accum_blocks && !timeout; ++b)
    {
      const unsigned long long* row = ctx->mailbox + (size_t)b * kMailboxStride;
      for (int v = 0; v < kAccumVals && !timeout; ++v)
      {
        unsigned long long g[2];
        for (int h = 0; h < 2 && !timeout; ++h)
          while (((g[h] = __atomic_load_n(row + 2 * v + h, __ATOMIC_RELAXED)) >> 32) != want)
          {
            if ((++spins & 0x3ff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) { timeout = true; break; }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
          }
        const unsigned long long bits = ((g[1] & 0xffffffffull) << 32) | (g[0] & 0xffffffffull);
        double d;
        std::memcpy(&d, &bits, sizeof(d));
        hp[v] += d;
      }
    }
    got = !timeout;
  }
  if (!got || ctx->mailbox_check)
  {
    double* dst = got ? ctx->host_pinned + 96 : hp;
    hipLaunchKernelGGL(k_accumulate_final, dim3(1), dim3(64), 0, st, ctx->partials, ctx->accum_blocks, ctx->reduce_out);
    LSA_HIP(ctx, hipMemcpyAsync(dst, ctx->reduce_out, kAccumVals * sizeof(double), hipMemcpyDeviceToHost, st));
    LSA_HIP(ctx, hipStreamSynchronize(st));
    // LSA_MAILBOX_CHECK: what came through the mailbox must be bit for bit what the device folds from its own partials
    if (got && std::memcmp(dst, hp, kAccumVals * sizeof(double)) != 0) return ctx->fail(LSA_E_STATE, "lsa_accumulate: mailbox and device fold disagree");
  }
  // the wheel odometer / gravity terms (lsa_set_sensor_terms) on top of the reduction, at the same rotation
  if (ctx->sensor_terms.wheel || ctx->sensor_terms.gravity)
    sensor_terms_add(ctx->sensor_terms, w, c.rot.R, c.rot.dRx, c.rot.dRy, c.rot.dRz, want_jacobian != 0, hp);
  *cost = hp[0];
  if (n_valid) *n_valid = (int)hp[28];
  if (g) for (int a = 0; a < 6; ++a) g[a] = hp[1 + a];
  if (H)
  {
    int h = 7;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) { H[a * 6 + b] = hp[h]; H[b * 6 + a] = hp[h]; ++h; }
  }
  return LSA_OK;
}

}  // extern "C"
