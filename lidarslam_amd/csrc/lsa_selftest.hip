// lsa_selftest.hip -- lsa_selftest_math: evaluates on the device the elementary operations the
// bit-exact CPU/GPU parity rests on (portable sin/cos/atan2/asin/acos of include/lsa_pmath.h, IEEE sqrt and
// division in float and double), so that a test can compare them bit for bit with the host.
// lsa_selftest_numerics: the fixed-size solvers built on them (PCA, eigen33, solve_spd, one residual block's
// normal equations, the pose algebra), evaluated by the very templates the kernels inline, one record per thread.
#include "lsa_accum.h"
#include "lsa_ctx.h"
#include "lsa_device_math.h"
#include "host/lsa_lm.h"

using namespace lsa;

namespace
{
__global__ void k_selftest(int fn, const double* __restrict__ x, const double* __restrict__ y, int n, double* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r = 0.;
  switch (fn)
  {
    case 0: r = lsa_sin(x[i]); break;
    case 1: r = lsa_cos(x[i]); break;
    case 2: r = lsa_atan2(y[i], x[i]); break;
    case 3: r = (double)sqrt_t((float)x[i]); break;
    case 4: r = (double)((float)x[i] / (float)y[i]); break;
    case 5: r = sqrt_t(x[i]); break;
    case 6: r = x[i] / y[i]; break;
    case 7: r = lsa_asin(x[i]); break;
    case 8: r = lsa_acos(x[i]); break;
  }
  out[i] = r;
}
}  // namespace

extern "C" int lsa_selftest_math(lsa_ctx* ctx, int fn, const double* x, const double* y, int n, double* out)
{
  if (!ctx || !x || !y || !out || n <= 0 || fn < 0 || fn > 8) return ctx ? ctx->fail(LSA_E_ARG, "lsa_selftest_math: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure_scratch(ctx, (size_t)n * 3 * sizeof(double));
  if (rc) return rc;
  double* dx = (double*)ctx->scratch_out;
  double* dy = dx + n;
  double* dout = dy + n;
  LSA_HIP(ctx, hipMemcpyAsync(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(dy, y, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_selftest, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fn, dx, dy, n, dout);
  LSA_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

// ---- lsa_selftest_numerics (record layouts: include/lidarslam_amd.h) ----
namespace
{
constexpr int kNumFns = 12;
// doubles per input / output record, by fn
constexpr int kNumIn[kNumFns] = {49, 49, 6, 6, 12, 42, 23, 42, 12, 42, 9, 36};
constexpr int kNumOut[kNumFns] = {15, 15, 12, 12, 4, 7, 28, 39, 4, 7, 12, 42};

template <typename T> __device__ __forceinline__ void put_eig(const Vec3<T>& e0, const Vec3<T>& e1, const Vec3<T>& e2, T l0, T l1, T l2, double* o)
{
  o[0] = l0; o[1] = l1; o[2] = l2;
  o[3] = e0.x; o[4] = e0.y; o[5] = e0.z;
  o[6] = e1.x; o[7] = e1.y; o[8] = e1.z;
  o[9] = e2.x; o[10] = e2.y; o[11] = e2.z;
}

template <typename T> __device__ __forceinline__ void probe_pca(const double* in, double* o)
{
  int k = (int)in[0];
  k = k < 1 ? 1 : (k > 16 ? 16 : k);
  CovAccum<T> acc;
  for (int p = 0; p < k; ++p) acc.add((float)in[1 + 3 * p], (float)in[2 + 3 * p], (float)in[3 + 3 * p]);
  Vec3<T> mean, e0, e1, e2;
  Sym3<T> cov;
  T l0, l1, l2;
  acc.finish(k, mean, cov);
  eigen33<T>(cov, e0, e1, e2, l0, l1, l2);
  o[0] = mean.x; o[1] = mean.y; o[2] = mean.z;
  put_eig(e0, e1, e2, l0, l1, l2, o + 3);
}

template <typename T> __device__ __forceinline__ void probe_eig33(const double* in, double* o)
{
  const Sym3<T> m = {(T)in[0], (T)in[1], (T)in[2], (T)in[3], (T)in[4], (T)in[5]};
  Vec3<T> e0, e1, e2;
  T l0, l1, l2;
  eigen33<T>(m, e0, e1, e2, l0, l1, l2);
  put_eig(e0, e1, e2, l0, l1, l2, o);
}

template <int N> __device__ __forceinline__ void probe_spd(const double* in, double* o)
{
  double A[N * N], b[N], x[N];
#pragma unroll
  for (int i = 0; i < N * N; ++i) A[i] = in[i];
#pragma unroll
  for (int i = 0; i < N; ++i) { b[i] = in[N * N + i]; x[i] = 0.; }
  o[0] = solve_spd<N>(A, b, x) ? 1. : 0.;
#pragma unroll
  for (int i = 0; i < N; ++i) o[1 + i] = x[i];
}

__device__ __forceinline__ void probe_accum(const double* in, double* o)
{
  const double* w = in + 17;
  RotConst c;
  rotation_and_derivatives(lsa_cos(w[3]), lsa_sin(w[3]), lsa_cos(w[4]), lsa_sin(w[4]), lsa_cos(w[5]), lsa_sin(w[5]), c.R, c.dRx, c.dRy, c.dRz);
  c.t[0] = w[0]; c.t[1] = w[1]; c.t[2] = w[2];
  double acc[kAccumVals];
#pragma unroll
  for (int v = 0; v < kAccumVals; ++v) acc[v] = 0.;
  accumulate_one(in, in[9], in[10], in[11], in[12], in[13], in[14], in[15], in[16] * in[16], c, true, acc);
#pragma unroll
  for (int v = 0; v < 28; ++v) o[v] = acc[v];
}

__device__ __forceinline__ void put_pose(const posemath::Pose& p, double* o)
{
  for (int r = 0; r < 3; ++r)
  {
    for (int c = 0; c < 3; ++c) o[r * 3 + c] = p(r, c);
    o[9 + r] = p(r, 3);
  }
}
__device__ __forceinline__ posemath::Pose get_pose(const double* in)
{
  posemath::Pose p = posemath::Pose::Identity();
  for (int r = 0; r < 3; ++r)
  {
    for (int c = 0; c < 3; ++c) p(r, c) = in[r * 3 + c];
    p(r, 3) = in[9 + r];
  }
  return p;
}
__device__ __forceinline__ void probe_pose(const double* in, double* o)
{
  using namespace posemath;
  const Pose M0 = get_pose(in), M1 = get_pose(in + 12);
  put_pose(FromXYZRPY(in + 24), o);
  ToXYZRPY(M0, o + 12);
  const Quaternion q = ToQuaternion(M0);
  o[18] = q.w; o[19] = q.x; o[20] = q.y; o[21] = q.z;
  const Quaternion qa = {in[30], in[31], in[32], in[33]}, qb = {in[34], in[35], in[36], in[37]};
  const Quaternion qs = Slerp(qa, qb, in[38]);
  o[22] = qs.w; o[23] = qs.x; o[24] = qs.y; o[25] = qs.z;
  o[26] = RotationAngle(M0);
  Rigid r;
  interp_eval(MakeInterpConst(M0, M1, in[40], in[41]), in[39], r);
  put_pose(FromRigid(r), o + 27);
}

__global__ void k_numerics(int fn, const double* __restrict__ in, int win, int n, double* __restrict__ out, int wout)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* a = in + (size_t)i * win;
  double* o = out + (size_t)i * wout;
  switch (fn)
  {
    case 0: probe_pca<float>(a, o); break;
    case 1: probe_pca<double>(a, o); break;
    case 2: probe_eig33<float>(a, o); break;
    case 3: probe_eig33<double>(a, o); break;
    case 4: probe_spd<3>(a, o); break;
    case 5: probe_spd<6>(a, o); break;
    case 6: probe_accum(a, o); break;
    case 7: probe_pose(a, o); break;
  }
}
}  // namespace

extern "C" int lsa_selftest_numerics(lsa_ctx* ctx, int fn, const double* in, int n, double* out)
{
  if (!in || !out || n <= 0 || fn < 0 || fn >= kNumFns) return ctx ? ctx->fail(LSA_E_ARG, "lsa_selftest_numerics: bad argument") : LSA_E_ARG;
  if (fn >= 8)  // the host twins: no device needed
  {
    const int N = (fn == 8 || fn == 10) ? 3 : 6;
    for (int i = 0; i < n; ++i)
    {
      const double* a = in + (size_t)i * kNumIn[fn];
      double* o = out + (size_t)i * kNumOut[fn];
      if (fn <= 9)
      {
        double x[6] = {0, 0, 0, 0, 0, 0};
        o[0] = host::ProbeSolveSPD(N, a, a + N * N, x) ? 1. : 0.;
        for (int k = 0; k < N; ++k) o[1 + k] = x[k];
      }
      else
        host::ProbeSymEigen(N, a, o, o + N);
    }
    return LSA_OK;
  }
  if (!ctx) return LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nin = (size_t)n * kNumIn[fn], nout = (size_t)n * kNumOut[fn];
  int rc = ensure_scratch(ctx, (nin + nout) * sizeof(double));
  if (rc) return rc;
  double* din = (double*)ctx->scratch_out;
  double* dout = din + nin;
  LSA_HIP(ctx, hipMemcpyAsync(din, in, nin * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_numerics, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, fn, din, kNumIn[fn], n, dout, kNumOut[fn]);
  LSA_HIP(ctx, hipGetLastError());
  LSA_HIP(ctx, hipMemcpyAsync(out, dout, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

// Diagnostic (scripts/clock_probe.py): `blocks` single-wave workgroups that sleep-spin for `ms` milliseconds of the
// constant 100 MHz wall clock on a stream of their own and then exit -- a load that occupies next to nothing, to see what the
// clock management of a mostly idle GPU does to the latency of the pipeline's short kernels.
__global__ void k_keep_busy(unsigned long long ticks)
{
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
extern "C" int lsa_selftest_keep_busy(lsa_ctx* ctx, int ms, int blocks)
{
  if (!ctx || ms < 0 || ms > 2000 || blocks < 1 || blocks > 256) return ctx ? ctx->fail(LSA_E_ARG, "lsa_selftest_keep_busy: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  static hipStream_t side = nullptr;
  if (!side) LSA_HIP(ctx, hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
  hipLaunchKernelGGL(k_keep_busy, dim3(blocks), dim3(64), 0, side, (unsigned long long)ms * 100000ull);
  return LSA_OK;
}
