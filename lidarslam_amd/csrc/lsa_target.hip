// lsa_target.hip -- the search grids of the match targets.  Replaces KDTreePCLAdaptor::Reset (nanoflann kd-tree build,
// slam_lib/include/LidarSlam/KDTreePCLAdaptor.h:57-65) by a three-level dense uniform grid, all pending targets in one
// launch sequence: bbox reduce -> cell count (wave-aggregated atomics on the coarse levels) -> exclusive scan ->
// cell-sorted float4 copies.  Also the lsa_*target* entry points that fill, stage ahead, adopt and read the targets.
// The grids are searched by lsa_match_fused.hip (production) and lsa_match_staged.hip (cross-check, overlap).
#include <cfloat>
#include "lsa_ctx.h"
#include "lsa_knn.h"
#include "lsa_match_internal.h"
#include "lsa_wave.h"

using namespace lsa;

namespace
{

// ------------------------------------------------------------------------------------------
// Search-grid construction.  Every target that changed since the last match (the two previous-scan targets
// of the ego-motion step, the two or three sub-maps after a keyframe) is built by ONE sequence of eight
// launches: blockIdx.y selects the target (point passes) or the (target, level) pair (cell passes).
constexpr int kBatchTargets = 6;
struct GridBatch
{
  int ntargets;
  int m[kBatchTargets];
  float cell_hint[kBatchTargets];
  const float4* pts[kBatchTargets];  // AoS points, two float4 per point
  float4* xyzl[kBatchTargets];
  int* bbox[kBatchTargets];
  GridDesc* desc[kBatchTargets];     // [kGridLevels] each
  uint32_t* cell_of[kBatchTargets][kGridLevels];
  uint32_t* cell_start[kBatchTargets][kGridLevels];
  uint32_t* cell_fill[kBatchTargets][kGridLevels];
  uint32_t* block_sums[kBatchTargets][kGridLevels];
  float4* sorted[kBatchTargets][kGridLevels];
};

__global__ __launch_bounds__(256) void k_target_prep(GridBatch gb)
{
  const int t = blockIdx.y;
  const int m = gb.m[t];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x * blockDim.x >= m) return;
  __shared__ float s_box[4][6];
  BoxF box;
  if (i < m)
  {
    const float4 a = gb.pts[t][2 * (size_t)i];
    const float4 b = gb.pts[t][2 * (size_t)i + 1];
    gb.xyzl[t][i] = make_float4(a.x, a.y, a.z, __uint_as_float(__float_as_uint(b.w) & 0xffffu));
    box = box_of_point(a.x, a.y, a.z);
  }
  box_block_send<4>(box, gb.bbox[t], s_box);
}

// desc[0]: cell = hint (grown until the grid fits its cell budget); every further level has cells 4 x
// larger (grown likewise).  One thread per target.  (Folded into k_grid_zero -- every workgroup deriving the geometry for
// itself -- it saved a launch and cost the zeroing 14 us: the launch covers the cell BUDGET, thousands of workgroups
// that mostly have nothing to zero then all walk the growth loop.)
__global__ void k_grid_setup(GridBatch gb)
{
  const int t = blockIdx.x;
  if (threadIdx.x != 0) return;
  const int* bbox = gb.bbox[t];
  float mn[3], mx[3];
  for (int d = 0; d < 3; ++d) { mn[d] = os2f(bbox[d]); mx[d] = os2f(bbox[3 + d]); }
  float cell = gb.cell_hint[t];
  for (int level = 0; level < kGridLevels; ++level)
  {
    const double cap = (double)grid_level_cells(level);
    if (level > 0) cell *= 4.0f;
    GridDesc g;
    while (true)
    {
      double total = 1;
      for (int d = 0; d < 3; ++d)
      {
        g.dims[d] = (int)floorf((mx[d] - mn[d]) / cell) + 1;
        total *= g.dims[d];
      }
      if (total <= cap) break;
      cell *= 1.26f;
    }
    for (int d = 0; d < 3; ++d) g.origin[d] = mn[d];
    g.cell = cell;
    g.inv_cell = 1.0f / cell;
    g.ncells = g.dims[0] * g.dims[1] * g.dims[2];
    g.npoints = gb.m[t];
    gb.desc[t][level] = g;
  }
}

__global__ __launch_bounds__(256) void k_grid_zero(GridBatch gb)
{
  const int t = blockIdx.y / kGridLevels, l = blockIdx.y % kGridLevels;
  const int nc = gb.desc[t][l].ncells;
  const int i0 = blockIdx.x * 1024 + threadIdx.x;
  if (blockIdx.x * 1024 > nc) return;
  uint32_t* cs = gb.cell_start[t][l];
  uint32_t* cf = gb.cell_fill[t][l];
#pragma unroll
  for (int q = 0; q < 4; ++q)
  {
    const int i = i0 + q * 256;
    if (i <= nc) cs[i] = 0;
    if (i < nc) cf[i] = 0;
  }
}

// Lanes of a wavefront that fall into the same cell are served by ONE atomic: the lowest of them adds the
// group's size, every member learns its rank inside the group.  Keypoints arrive in scan order, so
// neighbouring lanes share the cells of the coarse levels, whose few counters plain atomics would hammer
// from every wave (measured: 72 us per pass on a 33k-point scan, against 10 us).
struct CellGroup
{
  int leader;  // lane that issues the atomic for this lane's cell
  int rank;    // position of this lane among the lanes of its cell
  int count;   // lanes of the wavefront in this cell
};
__device__ __forceinline__ CellGroup group_by_cell(bool active, uint32_t cid)
{
  CellGroup g{-1, 0, 0};
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long remaining = __ballot(active);
  while (remaining)
  {
    const int first = __ffsll((long long)remaining) - 1;
    const uint32_t c = __shfl(cid, first);
    const unsigned long long same = __ballot(active && cid == c);
    if (active && cid == c)
    {
      g.leader = first;
      g.rank = __popcll(same & below);
      g.count = __popcll(same);
    }
    remaining &= ~same;
  }
  return g;
}

// one read of the point, its cell at every level
__global__ __launch_bounds__(256) void k_grid_count(GridBatch gb)
{
  const int t = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x * blockDim.x >= gb.m[t]) return;
  const bool active = i < gb.m[t];
  const float4 p = active ? gb.xyzl[t][i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int l = 0; l < kGridLevels; ++l)
  {
    const GridDesc g = gb.desc[t][l];
    const int cx = cell_coord(p.x, g.origin[0], g.inv_cell, g.dims[0]);
    const int cy = cell_coord(p.y, g.origin[1], g.inv_cell, g.dims[1]);
    const int cz = cell_coord(p.z, g.origin[2], g.inv_cell, g.dims[2]);
    const uint32_t cid = (uint32_t)((cz * g.dims[1] + cy) * g.dims[0] + cx);
    if (active) gb.cell_of[t][l][i] = cid;
    if (l == 0)
    {
      if (active) atomicAdd(&gb.cell_start[t][l][cid], 1u);
    }
    else
    {
      const CellGroup cg = group_by_cell(active, cid);
      if (active && lane == cg.leader) atomicAdd(&gb.cell_start[t][l][cid], (uint32_t)cg.count);
    }
  }
}

// exclusive scan of cell_start[0 .. ncells] in three passes (1024 elements per block)
__global__ __launch_bounds__(256) void k_scan_block(GridBatch gb)
{
  __shared__ uint32_t wsum[4];
  const int t = blockIdx.y / kGridLevels, l = blockIdx.y % kGridLevels;
  const int total = gb.desc[t][l].ncells + 1;
  const int base = blockIdx.x * 1024;
  if (base >= total) return;
  uint32_t* data = gb.cell_start[t][l];
  uint32_t v[4], tsum = 0;
  for (int q = 0; q < 4; ++q)
  {
    const int i = base + threadIdx.x * 4 + q;
    v[q] = (i < total) ? data[i] : 0;
    tsum += v[q];
  }
  uint32_t block_sum;
  uint32_t run = block_exclusive_scan<4>(tsum, wsum, &block_sum);
  for (int q = 0; q < 4; ++q)
  {
    const int i = base + threadIdx.x * 4 + q;
    if (i < total) data[i] = run;
    run += v[q];
  }
  if (threadIdx.x == 255) gb.block_sums[t][l][blockIdx.x] = block_sum;
}
// third pass fused into the second: every block sums the totals of the blocks in front of it itself (a grid of 4 M
// cells is 4 096 blocks: sixteen loads per thread)
__global__ __launch_bounds__(256) void k_scan_add(GridBatch gb)
{
  __shared__ uint32_t part[4];
  const int t = blockIdx.y / kGridLevels, l = blockIdx.y % kGridLevels;
  const int total = gb.desc[t][l].ncells + 1;
  const int base = blockIdx.x * 1024;
  if (base >= total) return;
  const uint32_t* sums = gb.block_sums[t][l];
  uint32_t mine = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += 256) mine += sums[j];
  const uint32_t add = block_reduce_all<4>(mine, OpSum(), part);
  uint32_t* data = gb.cell_start[t][l];
  for (int q = 0; q < 4; ++q)
  {
    const int i = base + threadIdx.x * 4 + q;
    if (i < total) data[i] += add;
  }
}

__global__ __launch_bounds__(256) void k_grid_scatter(GridBatch gb)
{
  const int t = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0)
  {
    // the bounding box is re-armed for the next build (its last readers were k_grid_zero's workgroups)
    int* bbox = gb.bbox[t];
    for (int d = 0; d < 3; ++d) { bbox[d] = kBoxLoArmedS; bbox[3 + d] = kBoxHiArmedS; }
  }
  if (blockIdx.x * blockDim.x >= gb.m[t]) return;
  const bool active = i < gb.m[t];
  const int lane = threadIdx.x & 63;
  const float4 p = active ? gb.xyzl[t][i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 rec = make_float4(p.x, p.y, p.z, __int_as_float(i));
#pragma unroll
  for (int l = 0; l < kGridLevels; ++l)
  {
    const uint32_t cid = active ? gb.cell_of[t][l][i] : 0u;
    uint32_t slot;
    if (l == 0)
      slot = active ? atomicAdd(&gb.cell_fill[t][l][cid], 1u) : 0u;
    else
    {
      const CellGroup cg = group_by_cell(active, cid);
      uint32_t base = 0;
      if (active && lane == cg.leader) base = atomicAdd(&gb.cell_fill[t][l][cid], (uint32_t)cg.count);
      slot = __shfl(base, max(cg.leader, 0)) + (uint32_t)cg.rank;
    }
    if (active) gb.sorted[t][l][gb.cell_start[t][l][cid] + slot] = rec;
  }
}

// builds the search grids of the listed targets, all in one sequence of launches on `st`
static int build_grids(lsa_ctx* ctx, const int* tis, int count, hipStream_t st)
{
  GridBatch gb;
  int nt = 0, max_m = 0, max_cells = 0;
  double bytes = 0;
  for (int i = 0; i < count; ++i)
  {
    Target& t = ctx->target[tis[i]];
    t.dirty = false;
    if (t.m == 0) continue;
    gb.m[nt] = t.m;
    gb.cell_hint[nt] = t.cell_hint;
    gb.pts[nt] = reinterpret_cast<const float4*>(t.pts);
    gb.xyzl[nt] = t.xyzl;
    gb.bbox[nt] = t.bbox_bits;
    gb.desc[nt] = t.desc;
    for (int l = 0; l < kGridLevels; ++l)
    {
      gb.cell_of[nt][l] = t.lv[l].cell_of;
      gb.cell_start[nt][l] = t.lv[l].cell_start;
      gb.cell_fill[nt][l] = t.lv[l].cell_fill;
      gb.block_sums[nt][l] = t.lv[l].block_sums;
      gb.sorted[nt][l] = t.lv[l].sorted;
      max_cells = std::max(max_cells, t.lv[l].max_cells);
    }
    max_m = std::max(max_m, t.m);
    bytes += (double)t.m * (32 + 16 + kGridLevels * (16 + 4 + 4 + 16 + 16));
    ++nt;
  }
  if (nt == 0) return LSA_OK;
  gb.ntargets = nt;
  ProfScope ps(ctx, st == ctx->stream ? "target_grid_build" : "target_grid_build_ahead", bytes, st);
  const int pb = (max_m + 255) / 256;
  const int cb = (max_cells + 1 + 1023) / 1024;  // the cell passes return at once beyond a grid's own cell count
  hipLaunchKernelGGL(k_target_prep, dim3(pb, nt), dim3(256), 0, st, gb);
  hipLaunchKernelGGL(k_grid_setup, dim3(nt), dim3(64), 0, st, gb);
  hipLaunchKernelGGL(k_grid_zero, dim3(cb, nt * kGridLevels), dim3(256), 0, st, gb);
  hipLaunchKernelGGL(k_grid_count, dim3(pb, nt), dim3(256), 0, st, gb);
  hipLaunchKernelGGL(k_scan_block, dim3(cb, nt * kGridLevels), dim3(256), 0, st, gb);
  hipLaunchKernelGGL(k_scan_add, dim3(cb, nt * kGridLevels), dim3(256), 0, st, gb);
  hipLaunchKernelGGL(k_grid_scatter, dim3(pb, nt), dim3(256), 0, st, gb);
  return LSA_OK;
}

// the (slot, type) pair of every target entry point names one of the six targets
bool valid_target(int slot, int type) { return slot >= 0 && slot <= 1 && type >= 0 && type <= 2; }

}  // namespace

namespace lsa
{
int build_target_grids(lsa_ctx* ctx, const int* tis, int count, hipStream_t st) { return build_grids(ctx, tis, count, st); }

// builds the search grids of every target marked dirty, on the context's stream
int flush_grids(lsa_ctx* ctx)
{
  int tis[6], n = 0;
  for (int ti = 0; ti < 6; ++ti)
    if (ctx->target[ti].dirty) tis[n++] = ti;
  return n ? build_grids(ctx, tis, n, ctx->stream) : LSA_OK;
}
}  // namespace lsa

extern "C" {

int lsa_set_target(lsa_ctx* ctx, int slot, int type, const lsa_point_t* pts, int m)
{
  if (!ctx || !valid_target(slot, type) || m < 0 || (!pts && m > 0)) return ctx ? ctx->fail(LSA_E_ARG, "lsa_set_target: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const int ti = slot * 3 + type;
  int rc = ensure_target(ctx, ti, m);
  if (rc) return rc;
  Target& t = ctx->target[ti];
  t.m = m;
  if (m == 0) return LSA_OK;
  {
    ProfScope ps(ctx, "target_upload_h2d", (double)m * 32);
    LSA_HIP(ctx, hipMemcpyAsync(t.pts, pts, (size_t)m * sizeof(lsa_point_t), hipMemcpyHostToDevice, ctx->stream));
  }
  t.dirty = true;  // the search grid is built with the other pending targets at the next match
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the host buffer may be pageable and go away
  return LSA_OK;
}

lsa_point_t* lsa_target_staging(lsa_ctx* ctx, int slot, int type, int capacity)
{
  if (!ctx || !valid_target(slot, type) || capacity < 0) return nullptr;
  const int ti = slot * 3 + type;
  if (capacity > ctx->tstage_cap[ti])
  {
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    retire_host(ctx, ctx->tstage[ti]);  // (a copy may still be reading it: freed at the next frame's start)
    ctx->tstage[ti] = nullptr;
    ctx->tstage_cap[ti] = 0;
    // the map grows keyframe after keyframe at the start of a sequence: doubling keeps the (slow) pinned
    // re-allocations to a handful
    const int cap = std::max(2 * capacity, 65536);
    if (hipHostMalloc((void**)&ctx->tstage[ti], (size_t)cap * sizeof(lsa_point_t), hipHostMallocDefault) != hipSuccess) return nullptr;
    ctx->tstage_cap[ti] = cap;
  }
  return ctx->tstage[ti];
}

int lsa_set_target_staged(lsa_ctx* ctx, int slot, int type, int m)
{
  if (!ctx || !valid_target(slot, type) || m < 0) return ctx ? ctx->fail(LSA_E_ARG, "lsa_set_target_staged: bad argument") : LSA_E_ARG;
  const int ti = slot * 3 + type;
  if (m > ctx->tstage_cap[ti]) return ctx->fail(LSA_E_STATE, "lsa_set_target_staged: more points than the staging buffer holds");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  if (slot == LSA_TARGET_MAP && ctx->map_ahead_ready[type])
  {
    // uploaded and built ahead on the look-ahead stream (lsa_stage_target_ahead): taken over when it is the same
    // staged cloud with the same cell size; either way its copy out of the staging buffer has to be over
    ctx->map_ahead_ready[type] = false;
    Target& spare = ctx->target[9 + type];
    if (m > 0 && spare.m == m && spare.cell_hint == ctx->target[ti].cell_hint)
    {
      std::swap(ctx->target[ti], spare);
      ctx->target[ti].dirty = false;
      ctx->map_ahead_adopted++;
      LSA_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_map_ahead[type], 0));
      return LSA_OK;
    }
    LSA_HIP(ctx, hipEventSynchronize(ctx->ev_map_ahead[type]));
  }
  int rc = ensure_target(ctx, ti, m);
  if (rc) return rc;
  Target& t = ctx->target[ti];
  t.m = m;
  if (m == 0) return LSA_OK;
  {
    ProfScope ps(ctx, "target_upload_h2d", (double)m * 32);
    LSA_HIP(ctx, hipMemcpyAsync(t.pts, ctx->tstage[ti], (size_t)m * sizeof(lsa_point_t), hipMemcpyHostToDevice, ctx->stream));
  }
  t.dirty = true;  // the search grid is built with the other pending targets at the next match
  return LSA_OK;
}

int lsa_stage_target_ahead(lsa_ctx* ctx, int slot, int type, int m)
{
  if (!ctx || slot != LSA_TARGET_MAP || !valid_target(slot, type) || m < 0) return ctx ? ctx->fail(LSA_E_ARG, "lsa_stage_target_ahead: bad argument") : LSA_E_ARG;
  const int ti = slot * 3 + type;
  if (m > ctx->tstage_cap[ti]) return ctx->fail(LSA_E_STATE, "lsa_stage_target_ahead: more points than the staging buffer holds");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->map_ahead_ready[type]) LSA_HIP(ctx, hipEventSynchronize(ctx->ev_map_ahead[type]));
  ctx->map_ahead_ready[type] = false;
  if (m == 0) return LSA_OK;
  int rc = ensure_target(ctx, 9 + type, m);
  if (rc) return rc;
  Target& t = ctx->target[9 + type];
  t.m = m;
  t.cell_hint = ctx->target[ti].cell_hint;
  LSA_HIP(ctx, hipMemcpyAsync(t.pts, ctx->tstage[ti], (size_t)m * sizeof(lsa_point_t), hipMemcpyHostToDevice, ctx->prefetch_stream));
  const int tis[1] = {9 + type};
  rc = build_grids(ctx, tis, 1, ctx->prefetch_stream);
  if (rc) return rc;
  LSA_HIP(ctx, hipEventRecord(ctx->ev_map_ahead[type], ctx->prefetch_stream));
  ctx->map_ahead_ready[type] = true;
  return LSA_OK;
}

int lsa_drop_target_ahead(lsa_ctx* ctx, int slot, int type)
{
  if (!ctx || slot != LSA_TARGET_MAP || !valid_target(slot, type)) return ctx ? ctx->fail(LSA_E_ARG, "lsa_drop_target_ahead: bad argument") : LSA_E_ARG;
  if (!ctx->map_ahead_ready[type]) return LSA_OK;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipEventSynchronize(ctx->ev_map_ahead[type]));  // the staging buffer is free to be rewritten after this
  ctx->map_ahead_ready[type] = false;
  return LSA_OK;
}

int lsa_staged_targets_adopted(const lsa_ctx* ctx) { return ctx ? ctx->map_ahead_adopted : 0; }

int lsa_set_target_from_set(lsa_ctx* ctx, int slot, int type, int set)
{
  if (!ctx || !valid_target(slot, type) || set < 0 || set > 2) return ctx ? ctx->fail(LSA_E_ARG, "lsa_set_target_from_set: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const int m = ctx->kp_n[set][type];
  const int ti = slot * 3 + type;
  if (slot == LSA_TARGET_PREVIOUS && set == LSA_SET_RAW_PREVIOUS && ctx->spare_ready[type])
  {
    // built ahead, beside the previous frame's registration (lsa_prepare_previous_targets): taken over if it still
    // describes this very set and was built with the cell size asked for now
    Target& spare = ctx->target[6 + type];
    ctx->spare_ready[type] = false;
    if (m > 0 && spare.m == m && ctx->spare_ver[type] == ctx->kp_ver[set][type] && spare.cell_hint == ctx->target[ti].cell_hint)
    {
      std::swap(ctx->target[ti], spare);
      ctx->target[ti].dirty = false;
      ctx->spare_adopted++;
      LSA_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_spare, 0));
      return LSA_OK;
    }
  }
  int rc = ensure_target(ctx, ti, m);
  if (rc) return rc;
  Target& t = ctx->target[ti];
  t.m = m;
  if (m == 0) return LSA_OK;
  LSA_HIP(ctx, hipMemcpyAsync(t.pts, ctx->kp[set][type], (size_t)m * sizeof(lsa_point_t), hipMemcpyDeviceToDevice, ctx->stream));
  t.dirty = true;
  return LSA_OK;
}

int lsa_prepare_previous_targets(lsa_ctx* ctx, unsigned type_mask)
{
  if (!ctx || (type_mask & ~7u)) return ctx ? ctx->fail(LSA_E_ARG, "lsa_prepare_previous_targets: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int tis[3], n = 0;
  for (int k = 0; k < 3; ++k)
  {
    ctx->spare_ready[k] = false;
    const int m = ctx->kp_n[LSA_SET_RAW_CURRENT][k];
    if (!((type_mask >> k) & 1u) || m <= 0) continue;
    int rc = ensure_target(ctx, 6 + k, m);
    if (rc) return rc;
    Target& t = ctx->target[6 + k];
    t.m = m;
    t.cell_hint = ctx->target[LSA_TARGET_PREVIOUS * 3 + k].cell_hint;
    tis[n++] = 6 + k;
  }
  if (n == 0) return LSA_OK;
  // the keypoints are final once everything enqueued so far has run; the copies and the grid build follow on the
  // look-ahead stream, beside whatever comes next on the context's stream
  LSA_HIP(ctx, hipEventRecord(ctx->ev_kp_ready, ctx->stream));
  LSA_HIP(ctx, hipStreamWaitEvent(ctx->prefetch_stream, ctx->ev_kp_ready, 0));
  for (int i = 0; i < n; ++i)
  {
    const int k = tis[i] - 6;
    LSA_HIP(ctx, hipMemcpyAsync(ctx->target[tis[i]].pts, ctx->kp[LSA_SET_RAW_CURRENT][k], (size_t)ctx->target[tis[i]].m * sizeof(lsa_point_t),
                                hipMemcpyDeviceToDevice, ctx->prefetch_stream));
  }
  int rc = build_grids(ctx, tis, n, ctx->prefetch_stream);
  if (rc) return rc;
  LSA_HIP(ctx, hipEventRecord(ctx->ev_spare, ctx->prefetch_stream));
  for (int i = 0; i < n; ++i)
  {
    const int k = tis[i] - 6;
    ctx->spare_ver[k] = ctx->kp_ver[LSA_SET_RAW_CURRENT][k];
    ctx->spare_ready[k] = true;
  }
  return LSA_OK;
}

int lsa_prepared_targets_adopted(const lsa_ctx* ctx) { return ctx ? ctx->spare_adopted : 0; }

int lsa_download_target(lsa_ctx* ctx, int slot, int type, lsa_point_t* out, int capacity)
{
  if (!ctx || !valid_target(slot, type) || !out) return ctx ? ctx->fail(LSA_E_ARG, "lsa_download_target: bad argument") : LSA_E_ARG;
  const Target& t = ctx->target[slot * 3 + type];
  const int n = std::min(capacity, t.m);
  if (n <= 0) return 0;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipMemcpyAsync(out, t.pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return n;
}

int lsa_target_size(const lsa_ctx* ctx, int slot, int type) { return (ctx && valid_target(slot, type)) ? ctx->target[slot * 3 + type].m : LSA_E_ARG; }

int lsa_set_target_cell_size(lsa_ctx* ctx, int slot, int type, float cell)
{
  if (!ctx || !valid_target(slot, type) || !(cell > 0.f)) return LSA_E_ARG;
  ctx->target[slot * 3 + type].cell_hint = cell;
  return LSA_OK;
}

}  // extern "C"
