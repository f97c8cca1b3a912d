// lsa_grid_submap.hip -- what leaves the device map: RollingGrid::Get, the bounding-box sub-maps that become kNN targets,
// and the sub-maps extracted ahead of time for a predicted box.  The data structure is described at the head of
// lsa_device_grid.hip.
#include <chrono>
#include "lsa_grid.h"
#include "lsa_device_grid_io.h"
#include "lsa_device_math.h"

using namespace lsa;

namespace
{
// "Ordered" = 0 (lsa_grid_order.hip): the extractions compact over r = 0 .. n-1 and read voxel perm[r]
template <typename P>
struct PermPred
{
  P p;
  const int* perm;
  __device__ bool operator()(int r) const { return p(perm[r]); }
};
template <typename E>
struct PermEmit
{
  E e;
  const int* perm;
  __device__ void operator()(int r, int at) const { e(perm[r], at); }
};

// ---- Get / BuildSubMapKdTree (RollingGrid.cxx:95-114, 353-442) ---------------------------------------------------------
// the outer voxels the box [mn, mx] touches (:365-370): PositionToVoxel of both corners against the grid position the
// device holds, clamped to the grid.  The box comes from the caller (floats) or from the bounding-box words the context's
// lsa_keypoint_bboxes_begin left on the device (ordered unsigned, 6 per keypoint type).  Every thread works it out for
// itself (a handful of operations against a launch of its own).
struct BoxArg { float mn[3], mx[3]; };
struct SubMapPred
{
  const u64* keys;
  const float4* pts;
  const unsigned* count;
  const int* st;
  BoxArg box;
  const unsigned* ctx_box;
  const int* range;  // non-null: lo[3], hi[3] in outer voxels, worked out before (the box of a sub-map extracted ahead)
  int grid_size;
  float resolution;
  double resolution_d;
  int mode;          // 0 every voxel in the box; 1 count >= min_frames or fixed; 2 the others (count < min_frames and not fixed), only if pass 1 was short
  unsigned min_frames;
  int min_points;
  int boxed;         // 0: the whole map (Get / BuildSubMapKdTree()), 3: count > min_frames (Get(clean))
  __device__ bool operator()(int i) const
  {
    if (boxed == 0) return true;
    if (boxed == 3) return count[i] > min_frames;
    int id = (int)(unsigned)(keys[i] >> 32);
    const int g = grid_size;
    const int z = id / (g * g); id -= z * g * g;
    const int y = id / g; const int x = id - y * g;
    const int c[3] = {x, y, z};
    if (range)
    {
#pragma unroll
      for (int d = 0; d < 3; ++d)
        if (c[d] < range[d] || c[d] > range[3 + d]) return false;
    }
    else
#pragma unroll
    for (int d = 0; d < 3; ++d)
    {
      const float lo_f = ctx_box ? ou2f(ctx_box[d]) : box.mn[d];
      const float hi_f = ctx_box ? ou2f(ctx_box[3 + d]) : box.mx[d];
      const float origin = __int_as_float(st[kStPosX + d]) - (float)((double)(g / 2) * resolution_d);
      const int lo = round_to_int((lo_f - origin) / resolution), hi = round_to_int((hi_f - origin) / resolution);
      if (c[d] < (lo > 0 ? lo : 0) || c[d] > (hi < g - 1 ? hi : g - 1)) return false;
    }
    if (mode == 0) return true;
    const unsigned label = (__float_as_uint(pts[2 * (size_t)i + 1].w) >> 24) & 0xffu;
    if (mode == 1) return count[i] >= min_frames || label == 1;
    return st[kStSubFirst] < min_points && count[i] < min_frames && label != 1;  // st[kStSubFirst]: what pass 1 kept
  }
};
struct PointEmit
{
  const float4* pts;
  float4* out;
  __device__ void operator()(int i, int at) const
  {
    out[2 * (size_t)at] = pts[2 * (size_t)i];
    out[2 * (size_t)at + 1] = pts[2 * (size_t)i + 1];
  }
};
// the outer voxels the box of `words` (ordered unsigned, lsa_keypoint_bboxes_begin) touches: lo[3], hi[3]
__device__ __forceinline__ void box_voxels(const unsigned* __restrict__ words, int grid_size, float resolution, double resolution_d, const int* __restrict__ st, int lo[3],
                                           int hi[3])
{
#pragma unroll
  for (int d = 0; d < 3; ++d)
  {
    const float origin = __int_as_float(st[kStPosX + d]) - (float)((double)(grid_size / 2) * resolution_d);
    const int a = round_to_int((ou2f(words[d]) - origin) / resolution), b = round_to_int((ou2f(words[3 + d]) - origin) / resolution);
    lo[d] = a > 0 ? a : 0;
    hi[d] = b < grid_size - 1 ? b : grid_size - 1;
  }
}
// sub-map ahead of time: the voxel range of the PREDICTED box is kept in the state ...
__global__ void k_pred_box(const unsigned* __restrict__ words, int grid_size, float resolution, double resolution_d, int* __restrict__ st)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int lo[3], hi[3];
  box_voxels(words, grid_size, resolution, resolution_d, st, lo, hi);
  for (int d = 0; d < 3; ++d) { st[kStPred + d] = lo[d]; st[kStPred + 3 + d] = hi[d]; }
}
// ... and compared with that of the ACTUAL box when the localization asks: the sub-map only depends on the range of
// outer voxels the box touches (RollingGrid.cxx:363-442).  {tag, same} goes to the host in one 8-byte store.
__global__ void k_box_check(const unsigned* __restrict__ words, int grid_size, float resolution, double resolution_d, int* __restrict__ st, u64* __restrict__ host_out,
                            unsigned tag)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int lo[3], hi[3];
  box_voxels(words, grid_size, resolution, resolution_d, st, lo, hi);
  bool same = true;
  for (int d = 0; d < 3; ++d) same = same && lo[d] == st[kStPred + d] && hi[d] == st[kStPred + 3 + d];
  if (same) st[kStUpdated] = 0;  // the sub-map that is about to be taken over is of the map as it is now
  __hip_atomic_store(host_out, ((u64)tag << 32) | (same ? 1u : 0u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// stable compaction of the map's voxels by pred, emit(voxel, position), in the grid's order
template <typename Pred, typename Emit>
void compact_map(lsa_device_grid* g, Pred pred, Emit emit, int* total, bool append = false, hipStream_t on = nullptr, u64* host_out = nullptr, unsigned host_tag = 0,
                 int* clear_flag = nullptr)
{
  if (g->Ordered) compact(g, pred, emit, g->st + kStN, g->n_upper, total, append, true, on, host_out, host_tag, clear_flag);
  else compact(g, PermPred<Pred>{pred, g->perm}, PermEmit<Emit>{emit, g->perm}, nullptr, g->order_n, total, append, true, on, host_out, host_tag, clear_flag);
}

// The sub-map of `pred` into `out` on `st`, in one pass or (filtered: MinFramesPerVoxel at work) in two; its size lands in
// st[kStSub] and, as {tag, size}, in *host_word behind the last kernel, which also takes `clear_flag` back (when given).
void extract_submap(lsa_device_grid* g, hipStream_t st, float4* out, SubMapPred pred, bool filtered, u64* host_word, unsigned tag, int* clear_flag, const char* scope)
{
  ProfScope ps(g->ctx, scope, (double)g->n_upper * 44, st);
  const PointEmit emit{pred.pts, out};
  pred.mode = filtered ? 1 : 0;
  compact_map(g, pred, emit, g->st + kStSub, false, st, filtered ? nullptr : host_word, tag, filtered ? nullptr : clear_flag);
  if (!filtered) return;
  // "Moving objects constraint was too strong, removing constraint": the rejected voxels follow when too few stayed
  pred.mode = 2;
  // the second pass appends behind what the first one kept (its predicate reads the first pass's count from a slot
  // of its own: the total moves while it runs)
  hipLaunchKernelGGL(k_copy_int, dim3(1), dim3(64), 0, st, g->st + kStSubFirst, g->st + kStSub);
  compact_map(g, pred, emit, g->st + kStSub, true, st, host_word, tag, clear_flag);
}

// bounded wait for the {tag, value} a kernel leaves in coherent host memory with ONE 8-byte store; false: it did not arrive
bool wait_tagged(const u64* word, unsigned tag, std::chrono::milliseconds timeout, u64* value)
{
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (true)
  {
    const u64 v = __atomic_load_n(word, __ATOMIC_ACQUIRE);
    if ((unsigned)(v >> 32) == tag) { *value = v & 0xffffffffull; return true; }
    if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > timeout) return false;
  }
}
}  // namespace

namespace lsa
{
// RollingGrid::Get(clean) left on the device: the points in the order lsa_device_grid_get hands them out, in the context's
// scratch buffer, *n of them; the grid's stream has been waited for
int grid_collect(lsa_device_grid* g, int clean, const lsa_point_t** pts, int* n)
{
  lsa_ctx* ctx = g->ctx;
  G_HIP(hipSetDevice(ctx->device));
  *pts = nullptr;
  *n = 0;
  if (g->n_upper == 0) return LSA_OK;
  int rc = ensure_map(g, g->n_upper);
  if (rc) return rc;
  rc = ensure_scratch(ctx, (size_t)g->n_upper * sizeof(lsa_point_t));
  if (rc) return rc;
  rc = g->Ordered ? LSA_OK : ensure_order(g);
  if (rc) return rc;
  const MapView m = g->buf[g->cur];
  rc = order_after_context(g);
  if (rc) return rc;
  SubMapPred pred{m.keys, m.pts, m.count, g->st, BoxArg{}, nullptr, nullptr, g->GridSize, (float)g->VoxelResolution, g->VoxelResolution, 0, g->MinFramesPerVoxel, -1, clean ? 3 : 0};
  compact_map(g, pred, PointEmit{m.pts, reinterpret_cast<float4*>(ctx->scratch_out)}, g->st + kStSub);
  int kept = 0;
  G_HIP(hipMemcpyAsync(&kept, g->st + kStSub, sizeof(int), hipMemcpyDeviceToHost, g->stream));
  G_HIP(hipStreamSynchronize(g->stream));
  *pts = static_cast<const lsa_point_t*>(ctx->scratch_out);
  *n = kept;
  return LSA_OK;
}
}  // namespace lsa

extern "C" {

// RollingGrid::Get(clean) (:95-114) in key order; returns the number of points written
int lsa_device_grid_get(lsa_device_grid* g, int clean, lsa_point_t* out, int capacity)
{
  if (!g || (!out && capacity > 0)) return LSA_E_ARG;
  const lsa_point_t* pts = nullptr;
  int kept = 0;
  const int rc = lsa::grid_collect(g, clean, &pts, &kept);  // (the scratch buffer is the context's; a sub-map extraction on its stream comes first too)
  if (rc) return rc;
  const int n = std::min(kept, capacity);
  if (n > 0) G_HIP(hipMemcpy(out, pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyDeviceToHost));
  return n;
}

// RollingGrid::BuildSubMapKdTree (:353-442): the sub-map becomes the kNN target (slot, type) of the context without
// leaving the device -- the points in key order, the search grid is built with the next match.  _begin enqueues it (on
// the grid's stream; the context's stream goes on behind it), _end waits for its size: several grids build side by
// side and are waited for once.  The box: mn/mx given; or, box_type >= 0, the box of that keypoint type as
// lsa_keypoint_bboxes_begin left it on the device (nothing is read back); or none: the whole map.
static int build_submap_begin(lsa_device_grid* g, const float mn[3], const float mx[3], int box_type, int min_nb_points, int slot, int type)
{
  if (!g || slot < 0 || slot > 1 || type < 0 || type > 2 || (mn && !mx) || box_type > 2)
    return g ? g->ctx->fail(LSA_E_ARG, "lsa_device_grid_build_submap: bad argument") : LSA_E_ARG;
  lsa_ctx* ctx = g->ctx;
  if (g->sub_target >= 0) return ctx->fail(LSA_E_STATE, "lsa_device_grid_build_submap_begin: the previous one has not been ended");
  G_HIP(hipSetDevice(ctx->device));
  const int ti = slot * 3 + type;
  g->sub_target = ti;
  g->submap_valid = true;
  tighten(g);
  if (g->n_upper == 0) return LSA_OK;
  int rc = ensure_map(g, g->n_upper);
  if (rc) return rc;
  rc = ensure_target(ctx, ti, g->n_upper);
  if (rc) return rc;
  rc = g->Ordered ? LSA_OK : ensure_order(g);
  if (rc) return rc;
  // The extraction runs on the CONTEXT's stream, behind the grid's last modification (ev_out): the box words, the target
  // and the next match are the context's anyway, so nothing else has to be ordered, and the size comes back through
  // coherent host memory -- no copy, no event, no host call between the kernels.
  hipStream_t st = ctx->stream;
  G_HIP(hipStreamWaitEvent(st, g->ev_out, 0));
  G_HIP(hipStreamWaitEvent(st, g->ev_ahead, 0));  // an extraction ahead of time that was not taken over shares the scratch
  g->ahead_phase = 0;
  const MapView m = g->buf[g->cur];
  const bool boxed = mn || box_type >= 0;
  SubMapPred pred{m.keys, m.pts, m.count, g->st, BoxArg{}, nullptr, nullptr, g->GridSize, (float)g->VoxelResolution, g->VoxelResolution, 0, g->MinFramesPerVoxel, min_nb_points, boxed ? 1 : 0};
  if (mn) for (int d = 0; d < 3; ++d) { pred.box.mn[d] = mn[d]; pred.box.mx[d] = mx[d]; }
  else if (boxed) pred.ctx_box = lsa::current_box_words(ctx) + 6 * box_type;
  const bool filtered = boxed && !(min_nb_points < 0 || g->MinFramesPerVoxel <= 1);
  // the sub-map is of the map as it is now: the changes the Adds before it flagged are in it (the flag goes with the
  // last kernel)
  extract_submap(g, st, reinterpret_cast<float4*>(ctx->target[ti].pts), pred, filtered, g->host_sub, ++g->sub_tag, g->st + kStUpdated, "map_submap");
  G_HIP(hipEventRecord(g->ev_sub, st));  // the grid's next modification comes behind the extraction
  g->sub_pending = true;
  return LSA_OK;
}
int lsa_device_grid_build_submap_begin(lsa_device_grid* g, const float mn[3], const float mx[3], int min_nb_points, int slot, int type)
{
  return build_submap_begin(g, mn, mx, -1, min_nb_points, slot, type);
}
int lsa_device_grid_build_submap_begin_for_keypoints(lsa_device_grid* g, int box_type, int min_nb_points, int slot, int type)
{
  if (box_type < 0) return g ? g->ctx->fail(LSA_E_ARG, "lsa_device_grid_build_submap_begin_for_keypoints: bad argument") : LSA_E_ARG;
  if (g) g->ctx->bbox_pending = false;  // the box stays on the device: no lsa_keypoint_bboxes_end follows
  return build_submap_begin(g, nullptr, nullptr, box_type, min_nb_points, slot, type);
}
int lsa_device_grid_build_submap_end(lsa_device_grid* g)
{
  if (!g) return LSA_E_ARG;
  lsa_ctx* ctx = g->ctx;
  if (g->sub_target < 0) return ctx->fail(LSA_E_STATE, "lsa_device_grid_build_submap_end: no lsa_device_grid_build_submap_begin before");
  G_HIP(hipSetDevice(ctx->device));
  Target& t = ctx->target[g->sub_target];
  g->sub_target = -1;
  int kept = 0;
  if (g->sub_pending)
  {
    g->sub_pending = false;
    // {tag, size} arrives as one 8-byte store (bounded wait: 2 s)
    u64 v = 0;
    if (!wait_tagged(g->host_sub, g->sub_tag, std::chrono::seconds(2), &v))
    {
      G_HIP(hipStreamSynchronize(ctx->stream));  // surfaces a failed launch as an error rather than a timeout
      return ctx->fail(LSA_E_HIP, "lsa_device_grid_build_submap_end: the sub-map's size did not arrive");
    }
    kept = (int)v;
  }
  // every refresh of the state enqueued before the extraction has landed (the extraction came behind ev_out)
  G_HIP(hipEventSynchronize(g->ev_state));
  t.m = kept;
  t.dirty = kept > 0;
  g->submap_count = kept;
  g->host_st[kStUpdated] = 0;
  return kept;
}
int lsa_device_grid_build_submap(lsa_device_grid* g, const float mn[3], const float mx[3], int min_nb_points, int slot, int type)
{
  const int rc = lsa_device_grid_build_submap_begin(g, mn, mx, min_nb_points, slot, type);
  return rc ? rc : lsa_device_grid_build_submap_end(g);
}

// ---- sub-maps ahead of time -------------------------------------------------------------------------------------------
// The sub-map the next localization will ask for only depends on the outer voxels its keypoints' box touches, and that box
// is known to a voxel long before the localization: _ahead_begin extracts the sub-map for the box of keypoint type
// `box_type` as lsa_keypoint_bboxes_begin(_interp) just left it on the device (the PREDICTED pose) into the context's
// spare map target, on the grid's stream behind the last insertion; _ahead_poll (non-blocking, call it now and then)
// enqueues the spare target's search grid once the extraction's size has arrived; _ahead_take, after
// lsa_keypoint_bboxes_begin under the ACTUAL pose, compares the two voxel ranges on the device and, when they are the
// same, swaps the spare target in as target (slot, type): *taken = 1, the return value is the sub-map's size, and
// lsa_device_grid_build_submap_begin / _end are not needed.  Anything that does not fit (*taken = 0) leaves everything
// as it was.  Same sub-map, byte for byte, either way.
int lsa_device_grid_submap_ahead_begin(lsa_device_grid* g, int box_type, int min_nb_points, int type)
{
  if (!g || box_type < 0 || box_type > 2 || type < 0 || type > 2) return g ? g->ctx->fail(LSA_E_ARG, "lsa_device_grid_submap_ahead_begin: bad argument") : LSA_E_ARG;
  lsa_ctx* ctx = g->ctx;
  G_HIP(hipSetDevice(ctx->device));
  g->ahead_phase = 0;
  ctx->bbox_pending = false;  // the box stays on the device
  tighten(g);
  if (g->n_upper == 0 || g->sub_target >= 0) return LSA_OK;
  int rc = ensure_map(g, g->n_upper);
  if (rc) return rc;
  if (ctx->map_ahead_ready[type]) { G_HIP(hipEventSynchronize(ctx->ev_map_ahead[type])); ctx->map_ahead_ready[type] = false; }
  rc = ensure_target(ctx, 9 + type, g->n_upper);
  if (rc) return rc;
  rc = after_submap(g);
  if (rc) return rc;
  rc = g->Ordered ? LSA_OK : ensure_order(g);  // behind the order of the last insertion, never an older one
  if (rc) return rc;
  // The box words: enqueued on this very stream by lsa_keypoint_boxes_predicted, or on the context's by
  // lsa_keypoint_bboxes_begin -- then this stream comes behind the context's.  (The spare target's last readers, searches of an
  // earlier frame, have long finished: every frame ends with the host reading its last solve's result.)
  if (!(ctx->pred_on_lookahead && g->stream == ctx->prefetch_stream))
  {
    rc = order_after_context(g);
    if (rc) return rc;
  }
  hipStream_t st = g->stream;
  // The predicted box becomes a range of outer voxels on the grid's stream, behind the last insertion (which may move the
  // grid).  The words are rewritten for the actual box later: should this kernel be so late that it reads those, or a
  // half-written box, the extraction below is simply for the range it stored, and _ahead_take compares the actual range
  // with the stored one -- a wrong guess costs the extraction, never the result.
  const unsigned* words = reinterpret_cast<const unsigned*>(ctx->range_bits + 16) + 6 * box_type;
  hipLaunchKernelGGL(k_pred_box, dim3(1), dim3(64), 0, st, words, g->GridSize, (float)g->VoxelResolution, g->VoxelResolution, g->st);
  const MapView m = g->buf[g->cur];
  const bool filtered = !(min_nb_points < 0 || g->MinFramesPerVoxel <= 1);
  const SubMapPred pred{m.keys, m.pts, m.count, g->st, BoxArg{}, nullptr, g->st + kStPred, g->GridSize, (float)g->VoxelResolution, g->VoxelResolution, 0,
                        g->MinFramesPerVoxel, min_nb_points, 1};
  extract_submap(g, st, reinterpret_cast<float4*>(ctx->target[9 + type].pts), pred, filtered, g->host_ahead, ++g->ahead_tag, nullptr, "map_submap_ahead");
  G_HIP(hipEventRecord(g->ev_ahead, st));  // whoever uses the grid's scratch next on another stream comes behind this
  g->ahead_phase = 1;
  g->ahead_type = type;
  g->ahead_min = min_nb_points;
  return LSA_OK;
}
int lsa_device_grid_submap_ahead_poll(lsa_device_grid* g)
{
  if (!g) return LSA_E_ARG;
  if (g->ahead_phase != 1) return g->ahead_phase;
  return lsa_device_grid_submap_ahead_poll_all(&g, 1);
}
// The same for several maps of one context at once: once ALL their sizes have arrived their search grids are built by ONE
// sequence of launches (a block row per target) instead of one sequence each.  Returns 1 while a size is missing, 2 when the
// grids are enqueued (or nothing was pending).
int lsa_device_grid_submap_ahead_poll_all(lsa_device_grid* const* grids, int count)
{
  if (!grids || count < 1 || count > 3) return LSA_E_ARG;
  lsa_ctx* ctx = nullptr;
  hipStream_t st = nullptr;
  u64 v[3];
  bool pending[3] = {false, false, false}, any = false;
  for (int i = 0; i < count; ++i)
  {
    lsa_device_grid* g = grids[i];
    if (!g) return LSA_E_ARG;
    if (g->ahead_phase != 1) continue;
    if (ctx && (g->ctx != ctx || g->stream != st)) return g->ctx->fail(LSA_E_ARG, "lsa_device_grid_submap_ahead_poll_all: maps of different contexts or streams");
    ctx = g->ctx;
    st = g->stream;
    v[i] = __atomic_load_n(g->host_ahead, __ATOMIC_ACQUIRE);
    if ((unsigned)(v[i] >> 32) != g->ahead_tag) return 1;
    pending[i] = any = true;
  }
  if (!any) return 2;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int tis[3], nt = 0;
  for (int i = 0; i < count; ++i)
  {
    if (!pending[i]) continue;
    lsa_device_grid* g = grids[i];
    const int type = g->ahead_type;
    Target& t = ctx->target[9 + type];
    g->ahead_m = (int)(unsigned)(v[i] & 0xffffffffull);
    t.m = g->ahead_m;
    t.cell_hint = ctx->target[LSA_TARGET_MAP * 3 + type].cell_hint;
    t.dirty = false;
    if (t.m > 0) tis[nt++] = 9 + type;
  }
  if (nt > 0)
  {
    const int rc = build_target_grids(ctx, tis, nt, st);
    if (rc) return rc;
  }
  for (int i = 0; i < count; ++i)
  {
    if (!pending[i]) continue;
    LSA_HIP(ctx, hipEventRecord(ctx->ev_map_ahead[grids[i]->ahead_type], st));
    grids[i]->ahead_phase = 2;
  }
  return 2;
}
// ... or waited for (a thread that has nothing else to do): returns once the search grid has been enqueued
int lsa_device_grid_submap_ahead_wait(lsa_device_grid* g)
{
  if (!g) return LSA_E_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  unsigned spins = 0;
  while (g->ahead_phase == 1)
  {
    const int rc = lsa_device_grid_submap_ahead_poll(g);
    if (rc < 0) return rc;
    if (rc == 1 && (++spins & 255u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500))
      return g->ctx->fail(LSA_E_HIP, "lsa_device_grid_submap_ahead_wait: the extraction's size did not arrive");
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return g->ahead_phase;
}
// _take in two steps, so that the comparisons of several maps are enqueued before any of them is waited for: _take_begin
// returns 1 when a comparison is on its way (0: nothing fits, extract the sub-map as usual), _take_end waits for it.
int lsa_device_grid_submap_ahead_take_begin(lsa_device_grid* g, int box_type, int min_nb_points, int slot, int type)
{
  if (!g || box_type < 0 || box_type > 2 || slot < 0 || slot > 1 || type < 0 || type > 2)
    return g ? g->ctx->fail(LSA_E_ARG, "lsa_device_grid_submap_ahead_take: bad argument") : LSA_E_ARG;
  lsa_ctx* ctx = g->ctx;
  g->take_pending = false;
  if (g->ahead_phase == 1)
  {
    const int rc = lsa_device_grid_submap_ahead_poll(g);
    if (rc < 0) return rc;
  }
  const bool fits = g->ahead_phase == 2 && g->ahead_type == type && g->ahead_min == min_nb_points && g->sub_target < 0 &&
                    ctx->target[9 + type].cell_hint == ctx->target[slot * 3 + type].cell_hint;
  g->ahead_phase = 0;
  if (!fits) return 0;
  G_HIP(hipSetDevice(ctx->device));
  // the comparison runs on the context's stream, where the actual box was just enqueued, behind the grid's stream (the
  // predicted range and the state it reads)
  G_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_map_ahead[type], 0));
  const unsigned tag = ++g->ahead_tag;
  const unsigned* words = lsa::current_box_words(ctx) + 6 * box_type;
  hipLaunchKernelGGL(k_box_check, dim3(1), dim3(64), 0, ctx->stream, words, g->GridSize, (float)g->VoxelResolution, g->VoxelResolution, g->st, g->host_ahead + 1, tag);
  g->take_pending = true;
  g->take_slot = slot;
  return 1;
}
int lsa_device_grid_submap_ahead_take_end(lsa_device_grid* g, int* taken)
{
  if (!g || !taken) return LSA_E_ARG;
  *taken = 0;
  if (!g->take_pending) return LSA_OK;
  g->take_pending = false;
  lsa_ctx* ctx = g->ctx;
  const int type = g->ahead_type, slot = g->take_slot;
  u64 v = 0;
  if (!wait_tagged(g->host_ahead + 1, g->ahead_tag, std::chrono::seconds(2), &v))
  {
    G_HIP(hipStreamSynchronize(ctx->stream));
    return ctx->fail(LSA_E_HIP, "lsa_device_grid_submap_ahead_take: the comparison did not arrive");
  }
  if (!(v & 1ull)) return LSA_OK;  // another range of voxels: the caller extracts the sub-map now
  ctx->bbox_pending = false;
  std::swap(ctx->target[slot * 3 + type], ctx->target[9 + type]);
  ctx->target[slot * 3 + type].dirty = false;
  g->submap_valid = true;
  g->submap_count = g->ahead_m;
  G_HIP(hipEventSynchronize(g->ev_state));  // the flag's last refresh has landed: it was taken back by the comparison
  g->host_st[kStUpdated] = 0;
  G_HIP(hipEventRecord(g->ev_sub, ctx->stream));
  *taken = 1;
  return g->ahead_m;
}
int lsa_device_grid_submap_ahead_take(lsa_device_grid* g, int box_type, int min_nb_points, int slot, int type, int* taken)
{
  if (!taken) return LSA_E_ARG;
  *taken = 0;
  const int rc = lsa_device_grid_submap_ahead_take_begin(g, box_type, min_nb_points, slot, type);
  return rc <= 0 ? rc : lsa_device_grid_submap_ahead_take_end(g, taken);
}

// RollingGrid::IsSubMapKdTreeValid(): an Add that changed a voxel's point has dropped the sub-map (RollingGrid.cxx:315-317);
// rolling and decay do not (as in the reference).  Waits for the modifications enqueued so far.
int lsa_device_grid_submap_valid(lsa_device_grid* g)
{
  if (!g) return 0;
  if (hipSetDevice(g->ctx->device) != hipSuccess || hipEventSynchronize(g->ev_state) != hipSuccess) return 0;
  if (g->host_st[kStUpdated]) g->submap_valid = false;  // the flag is taken back by the next sub-map (lsa_device_grid_build_submap_begin)
  return g->submap_valid && g->submap_count > 0 ? 1 : 0;  // an empty sub-map counts as invalid (RollingGrid.h:154)
}

}  // extern "C"
