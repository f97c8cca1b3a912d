// lsa_compact.h -- the one stable compaction of the library: the device maps' (lsa_device_grid.hip, lsa_grid_submap.hip) and the frame
// converters' (lsa_wire.hip).  What stays is a predicate functor bool(int i), what happens to it an emitter functor
// void(int i, int position).  One (predicate, emitter) pair is launched from ONE translation unit only: the kernel would
// exist twice in the library otherwise.
#pragma once
#include <algorithm>
#include <hip/hip_runtime.h>
#include "lsa_wave.h"

namespace lsa
{
typedef unsigned long long u64;

// ---- stable compaction: chunk counts -> scatter (the predicate is evaluated twice) ---------------------------------------
// Two launches: every scatter block sums the counts of the chunks before it itself (a map of a few hundred thousand voxels
// is a few hundred chunks), the last block leaves the total.
template <typename Pred>
__global__ __launch_bounds__(256) void k_compact_count(Pred pred, const int* __restrict__ n_ptr, int n_fixed, int* __restrict__ chunk_count)
{
  __shared__ int cnt[4];
  const int n = n_ptr ? *n_ptr : n_fixed;
  if (blockIdx.x * 1024 >= n) { if (threadIdx.x == 0) chunk_count[blockIdx.x] = 0; return; }
  int mine = 0;
  for (int q = 0; q < 4; ++q)
  {
    const int i = blockIdx.x * 1024 + q * 256 + threadIdx.x;
    if (i < n && pred(i)) ++mine;
  }
  mine = block_reduce<4>(mine, OpSum(), cnt);
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = mine;
}
// total_out: where the number kept goes (never the word n_ptr points at: the other blocks still read that one);
// base_ptr: the output starts behind *base_ptr elements (appending), at 0 when null
template <typename Pred, typename Emit>
__global__ __launch_bounds__(256) void k_compact_scatter(Pred pred, Emit emit, const int* __restrict__ n_ptr, int n_fixed, const int* __restrict__ chunk_count,
                                                         const int* __restrict__ base_ptr, int* __restrict__ total_out,
                                                         u64* __restrict__ host_out = nullptr, unsigned host_tag = 0, int* __restrict__ clear_flag = nullptr)
{
  __shared__ int wave_cnt[4];
  __shared__ int before[4];
  const int n = n_ptr ? *n_ptr : n_fixed;
  const bool last = blockIdx.x == gridDim.x - 1;
  if (blockIdx.x * 1024 >= n && !last) return;
  int mine = 0;
  for (int c = threadIdx.x; c < (int)blockIdx.x; c += 256) mine += chunk_count[c];
  int run = (base_ptr ? *base_ptr : 0) + block_reduce_all<4>(mine, OpSum(), before);
  for (int q = 0; q < 4; ++q)
  {
    const int i = blockIdx.x * 1024 + q * 256 + threadIdx.x;
    const bool keep = i < n && pred(i);
    const u64 ballot = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();  // wave_cnt of the round before has been read
    if (lane == 0) wave_cnt[wv] = __popcll(ballot);
    __syncthreads();
    int base = run;
    for (int w = 0; w < wv; ++w) base += wave_cnt[w];
    if (keep) emit(i, base + __popcll(ballot & ((1ull << lane) - 1ull)));
    run += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  }
  if (last && threadIdx.x == 0)
  {
    *total_out = run;
    if (clear_flag) *clear_flag = 0;
    // the total for the host: tag and count in ONE 8-byte store into coherent host memory (no copy, no event)
    if (host_out) __hip_atomic_store(host_out, ((u64)host_tag << 32) | (u64)(unsigned)run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
__global__ void k_copy_int(int* __restrict__ dst, const int* __restrict__ src);  // defined once, in lsa_device_grid.hip

// stable compaction of [0, n) (n on the device when n_ptr is given) by pred, emit(i, position), on `st`; the number kept
// lands in *total (added to what is there when `append`).  chunks: room for the counts of the chunks of 1024, one at
// least; aside_slot: a device word of the caller's for the total on its way (only read when compacting in place or appending)
template <typename Pred, typename Emit>
void stable_compact(hipStream_t st, int* chunks, int* aside_slot, Pred pred, Emit emit, const int* n_ptr, int n_bound, int* total, bool append = false,
                    bool copy_back = true, u64* host_out = nullptr, unsigned host_tag = 0, int* clear_flag = nullptr)
{
  const int nchunks = std::max((n_bound + 1023) / 1024, 1);
  hipLaunchKernelGGL((k_compact_count<Pred>), dim3(nchunks), dim3(256), 0, st, pred, n_ptr, n_bound, chunks);
  // compacting in place of the count it reads (Roll, ClearOldPoints), or appending behind it: the blocks of the
  // scatter still read the old count, the new one waits in a slot of its own until they are through
  const bool aside = n_ptr == total || append;
  int* const sum = aside ? aside_slot : total;
  hipLaunchKernelGGL((k_compact_scatter<Pred, Emit>), dim3(nchunks), dim3(256), 0, st, pred, emit, n_ptr, n_bound, chunks, append ? total : (const int*)nullptr, sum,
                     host_out, host_tag, clear_flag);
  if (aside && copy_back) hipLaunchKernelGGL(k_copy_int, dim3(1), dim3(64), 0, st, total, sum);  // otherwise the caller's next kernel takes it from the slot
}
}  // namespace lsa
