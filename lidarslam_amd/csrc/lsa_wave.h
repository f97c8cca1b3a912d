// lsa_wave.h -- the lane-level glue of the kernels (internal): wavefront and workgroup reductions and scans, the
// order-preserving codings of floats and doubles, and the boxes that are reduced into armed words with atomics.  Device-only
// apart from the codings.  The shapes are part of the contract: a reduction is the __shfl_down tree 32, 16, ... 1 with
// v = op(v, shuffled), a workgroup's combine runs over the wavefronts left to right, ((s0 op s1) op s2) op s3 -- integer
// results do not depend on either, k_overlap_score's float sum does and is compared bit for bit.
// Outside on purpose (hot path or another shape, each with tests of its own): the DPP group scans of lsa_match_fused.hip /
// lsa_knn.h, the sub-wavefront group scan of lsa_match_staged.hip, lsa_accum.h, lsa_lm.hip.
#pragma once
#include <cfloat>
#include <hip/hip_runtime.h>

namespace lsa
{
// ---- operations ----------------------------------------------------------------------------------------------------------
struct OpSum
{
  template <typename T> __device__ T operator()(T a, T b) const { return a + b; }
};
// (floats: fminf / fmaxf, which ignore a NaN; everything else by comparison)
struct OpMin
{
  template <typename T> __device__ T operator()(T a, T b) const { return b < a ? b : a; }
  __device__ float operator()(float a, float b) const { return fminf(a, b); }
  __device__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct OpMax
{
  template <typename T> __device__ T operator()(T a, T b) const { return b > a ? b : a; }
  __device__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

// ---- reductions ----------------------------------------------------------------------------------------------------------
// lane 0 holds the result (int, unsigned, long long, unsigned long long, float, double)
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op)
{
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_down(v, o));
  return v;
}
template <typename T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, OpSum()); }
template <typename T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, OpMin()); }
template <typename T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, OpMax()); }

// The arg-min of (value, index) pairs, index -1: none.  before(v2, i2, v, i) says that (v2, i2) ranks before (v, i) and
// must be a total order: then any tree gives the sequential loop's answer.  argmin_take is one step of that loop.
template <typename Before>
__device__ __forceinline__ void argmin_take(float& v, int& i, float v2, int i2, Before before)
{
  if (i2 >= 0 && (i < 0 || before(v2, i2, v, i))) { v = v2; i = i2; }
}
// lane 0 holds the result
template <typename Before>
__device__ __forceinline__ void wave_argmin(float& v, int& i, Before before)
{
  for (int o = 32; o > 0; o >>= 1)
  {
    const float v2 = __shfl_down(v, o);
    const int i2 = __shfl_down(i, o);
    argmin_take(v, i, v2, i2, before);
  }
}

// EVERY thread of the workgroup (WAVES wavefronts) must call it; scratch: the caller's __shared__ array of WAVES elements,
// not to be used again before the workgroup's next barrier.  One barrier; thread 0 holds the result.
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T block_reduce(T v, Op op, T* scratch)
{
  v = wave_reduce(v, op);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
  {
    v = scratch[0];
    for (int w = 1; w < WAVES; ++w) v = op(v, scratch[w]);
  }
  return v;
}
// ... every thread holds the result
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T block_reduce_all(T v, Op op, T* scratch)
{
  v = wave_reduce(v, op);
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  v = scratch[0];
  for (int w = 1; w < WAVES; ++w) v = op(v, scratch[w]);
  return v;
}

// ---- scans (sums) --------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_inclusive_scan(T v)
{
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1)
  {
    const T t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  return v;
}
// The sum of v over the threads in front of this one.  EVERY thread of the workgroup must call it; scratch as above; one
// barrier.  *total (when asked for): the sum over the workgroup, which must then consist of all WAVES wavefronts.
template <int WAVES, typename T>
__device__ __forceinline__ T block_exclusive_scan(T v, T* scratch, T* total = nullptr)
{
  const T inc = wave_inclusive_scan(v);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) scratch[wave] = inc;
  __syncthreads();
  T before = 0;
  for (int w = 0; w < wave; ++w) before += scratch[w];
  if (total)
  {
    T all = scratch[0];
    for (int w = 1; w < WAVES; ++w) all += scratch[w];
    *total = all;
  }
  return before + inc - v;
}

// ---- order-preserving codings --------------------------------------------------------------------------------------------
// Two conventions for floats, kept apart by their names because their armed words differ.
//   unsigned (f2ou / ou2f): for atomicMin / atomicMax on unsigned words, armed kBoxLoArmed / kBoxHiArmed; no float but a
//                           NaN codes to either
//   signed   (f2os / os2f): the device maps' int st[] words, the targets' boxes, lsa_device_grid_roll's host box; armed
//                           kBoxLoArmedS / kBoxHiArmedS
__host__ __device__ __forceinline__ unsigned f2ou(float f)
{
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float ou2f(unsigned u) { return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
__host__ __device__ __forceinline__ int f2os(float f)
{
  const int i = __builtin_bit_cast(int, f);
  return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __device__ __forceinline__ float os2f(int i) { return __builtin_bit_cast(float, i >= 0 ? i : i ^ 0x7fffffff); }
// doubles, the unsigned convention: armed ~0ull / 0ull
__host__ __device__ __forceinline__ unsigned long long d2ou(double d)
{
  const unsigned long long u = __builtin_bit_cast(unsigned long long, d);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double ou2d(unsigned long long u)
{
  return __builtin_bit_cast(double, (u & 0x8000000000000000ull) ? (u & 0x7fffffffffffffffull) : ~u);
}
constexpr unsigned kBoxLoArmed = ~0u, kBoxHiArmed = 0u;
constexpr int kBoxLoArmedS = 0x7fffffff, kBoxHiArmedS = (int)0x80000000;

// arms the boxes of the three keypoint types: 18 words, lo[3] hi[3] per type (defined once, in lsa_transform.hip)
__global__ void k_box_arm(unsigned* __restrict__ words);

// ---- boxes in unsigned words ---------------------------------------------------------------------------------------------
struct BoxU
{
  unsigned lo[3] = {kBoxLoArmed, kBoxLoArmed, kBoxLoArmed}, hi[3] = {kBoxHiArmed, kBoxHiArmed, kBoxHiArmed};
};
// a NaN coordinate takes no part, as in a min / max loop written with comparisons
__device__ __forceinline__ void box_take(BoxU& b, float x, float y, float z)
{
  const float v[3] = {x, y, z};
  for (int d = 0; d < 3; ++d)
    if (v[d] == v[d])
    {
      const unsigned u = f2ou(v[d]);
      b.lo[d] = u < b.lo[d] ? u : b.lo[d];
      b.hi[d] = u > b.hi[d] ? u : b.hi[d];
    }
}
// words: lo[3], hi[3].  The wavefront's box: six atomics by its first lane
__device__ __forceinline__ void box_wave_send(BoxU b, unsigned* __restrict__ words)
{
  for (int d = 0; d < 3; ++d) { b.lo[d] = wave_min(b.lo[d]); b.hi[d] = wave_max(b.hi[d]); }
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 3; ++d) { atomicMin(&words[d], b.lo[d]); atomicMax(&words[3 + d], b.hi[d]); }
}
// The workgroup's box: six atomics a workgroup (every wavefront aiming at the same six words was 15 us for 27 k points), none
// for a word still as it was armed.  EVERY thread of the workgroup must call it; scratch: __shared__ unsigned [WAVES][6].
template <int WAVES>
__device__ __forceinline__ void box_block_send(BoxU b, unsigned* __restrict__ words, unsigned (*scratch)[6])
{
  for (int d = 0; d < 3; ++d) { b.lo[d] = wave_min(b.lo[d]); b.hi[d] = wave_max(b.hi[d]); }
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 3; ++d) { scratch[threadIdx.x >> 6][d] = b.lo[d]; scratch[threadIdx.x >> 6][3 + d] = b.hi[d]; }
  __syncthreads();
  if (threadIdx.x < 6)
  {
    const int d = threadIdx.x;
    unsigned v = scratch[0][d];
    for (int w = 1; w < WAVES; ++w) v = d < 3 ? OpMin()(v, scratch[w][d]) : OpMax()(v, scratch[w][d]);
    if (d < 3) { if (v != kBoxLoArmed) atomicMin(&words[d], v); }
    else if (v != kBoxHiArmed) atomicMax(&words[d], v);
  }
}

// ---- the float twin: boxes of raw points in signed words -------------------------------------------------------------------
// fminf / fmaxf on the floats, coded only at the atomic (fminf ignores a NaN where the coding would rank it)
struct BoxF
{
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
};
__device__ __forceinline__ BoxF box_of_point(float x, float y, float z)
{
  BoxF b;
  b.lo[0] = b.hi[0] = x; b.lo[1] = b.hi[1] = y; b.lo[2] = b.hi[2] = z;
  return b;
}
// EVERY thread of the workgroup must call it; scratch: __shared__ float [WAVES][6]; six atomics a workgroup
template <int WAVES>
__device__ __forceinline__ void box_block_send(BoxF b, int* __restrict__ words, float (*scratch)[6])
{
  for (int d = 0; d < 3; ++d) { b.lo[d] = wave_min(b.lo[d]); b.hi[d] = wave_max(b.hi[d]); }
  if ((threadIdx.x & 63) == 0)
    for (int d = 0; d < 3; ++d) { scratch[threadIdx.x >> 6][d] = b.lo[d]; scratch[threadIdx.x >> 6][3 + d] = b.hi[d]; }
  __syncthreads();
  if (threadIdx.x < 6)
  {
    const int d = threadIdx.x;
    float v = scratch[0][d];
    for (int w = 1; w < WAVES; ++w) v = d < 3 ? fminf(v, scratch[w][d]) : fmaxf(v, scratch[w][d]);
    if (d < 3) atomicMin(&words[d], f2os(v));
    else atomicMax(&words[d], f2os(v));
  }
}
}  // namespace lsa
