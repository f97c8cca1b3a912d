// lsa_device_grid.hip -- LidarSlam::RollingGrid (slam_lib/include/LidarSlam/RollingGrid.h:63-212,
// slam_lib/src/RollingGrid.cxx) resident on the device: voxel insertion with the sampling modes, rolling,
// decay, bounding-box sub-map extraction straight into a kNN target.  SURVEY.md 8f-1.
//
// The reference keeps the map as unordered_map<outer voxel, unordered_map<leaf voxel, Voxel>>.  Here the map is ONE
// array of voxels sorted by the 64-bit key (outer index << 32 | leaf index) -- keys, points and counts in three
// parallel arrays, double-buffered:
//   Add      the batch is keyed and sorted by (key, arrival order) (runs sorted by a workgroup each, merged by rank); the
//            first thread of a run of equal keys finds the voxel by binary search and folds the run's points for it IN
//            ARRIVAL ORDER through the reference's per-point rule (FIRST / LAST / MAX_INTENSITY / CENTER_POINT, fixed
//            points, one count per Add call), exactly what the sequential loop of RollingGrid.cxx:183-312 does to that
//            voxel; new voxels are merged in by rank (two binary searches, one scatter) -- no hash table, no atomics on
//            voxels; seven launches for all the maps of a keyframe together
//   Roll     a shift of the outer coordinates keeps the key order: folded into Add's merge (on its own: transform + stable
//            compaction)
//   decay    ClearOldPoints: stable compaction
//   sub-map  voxels whose outer index lies in the box, stable compaction straight into the target's point buffer
// Iteration order.  The reference's Get / BuildSubMapKdTree hand the points out in libstdc++'s hash iteration order,
// an accident of the container.  Two orders, chosen by "Ordered" (the host RollingGrid's SetOrdered):
//   1 (default)  KEY ORDER (outer index, then leaf index as unsigned) -- the order of the array itself; the oracle and
//                the host RollingGrid use it too: a defined order in place of an accidental one
//   0            the reference's container order.  Every modification leaves a record of what it did to the key set
//                (the keys an Add created, in first-arrival order; the offset of a roll; the keys ClearOldPoints
//                erased), copied to the host behind it; the host replays the records on a keys-only copy of the
//                reference's containers (host/lsa_map_order.h) and uploads the keys in their iteration order before the
//                next extraction; a kernel turns them into places in the sorted array (binary search), and the
//                extractions compact over that permutation instead of over the array.  The points never leave the
//                device.
// Nothing here waits for the device except the calls that return a size or points to the host.
//
// One job per unit (lsa_grid.h is what they share): this one keeps the lifecycle and the parameters, Roll and decay;
// Add, its staging and entry points are in lsa_grid_add.hip; the records and the permutation of "Ordered" = 0 in
// lsa_grid_order.hip; Get, the sub-maps and the sub-maps extracted ahead of time in lsa_grid_submap.hip.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "lsa_grid.h"
#include "lsa_device_grid_io.h"
#include "lsa_device_math.h"

using namespace lsa;

namespace lsa
{
__global__ void k_copy_int(int* __restrict__ dst, const int* __restrict__ src) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = *src; }  // lsa_compact.h
}  // namespace lsa

namespace
{
// ---- Roll (RollingGrid.cxx:117-157) --------------------------------------------------------------------------------
// how many outer voxels the grid has to move so that the box fits (one thread); explicit box: roll_to != nullptr
__global__ void k_roll_decide(GridParams p, int* __restrict__ st, int use_box)
{
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double halfGridSize = static_cast<double>(p.grid_size) / 2 * p.resolution_d;
  const float h = (float)halfGridSize;
  for (int d = 0; d < 3; ++d)
  {
    int off = 0;
    if (use_box)
    {
      const float mnv = os2f(st[kStTmp + d]), mxv = os2f(st[kStTmp + 3 + d]);
      const float pos = __int_as_float(st[kStPosX + d]);
      const float down = mnv - (pos - h);
      const float up = mxv - (pos + h);
      float o = (up + down) / 2.f;
      const float lo = fminf(down, 0.f), hi = fmaxf(up, 0.f);
      o = fminf(fmaxf(o, lo), hi);
      off = round_to_int(o / p.resolution);
    }
    st[kStOff + d] = off;
    st[kStPosX + d] = __float_as_int(__int_as_float(st[kStPosX + d]) + (float)off * p.resolution);
  }
  // re-arm the box for the next batch
  for (int d = 0; d < 3; ++d) { st[kStTmp + d] = kBoxLoArmedS; st[kStTmp + 3 + d] = kBoxHiArmedS; }
}
struct RollPred
{
  const u64* keys;
  const int* st;
  int grid_size;
  __device__ bool shifted(int i, u64& out) const
  {
    const u64 k = keys[i];
    int id = (int)(unsigned)(k >> 32);
    const int g = grid_size;
    int z = id / (g * g);
    id -= z * g * g;
    int y = id / g;
    int x = id - y * g;
    x -= st[kStOff + 0]; y -= st[kStOff + 1]; z -= st[kStOff + 2];
    if (x < 0 || y < 0 || z < 0 || x >= g || y >= g || z >= g) return false;
    out = ((u64)(unsigned)(z * g * g + y * g + x) << 32) | (k & 0xffffffffull);
    return true;
  }
  __device__ bool operator()(int i) const { u64 o; return shifted(i, o); }
};
struct RollEmit
{
  RollPred pred;
  MapView src, dst;
  __device__ void operator()(int i, int at) const
  {
    u64 k;
    pred.shifted(i, k);
    dst.keys[at] = k;
    dst.pts[2 * (size_t)at] = src.pts[2 * (size_t)i];
    dst.pts[2 * (size_t)at + 1] = src.pts[2 * (size_t)i + 1];
    dst.count[at] = src.count[i];
  }
};
__global__ void k_after_roll(int* __restrict__ st)
{
  if (threadIdx.x == 0 && blockIdx.x == 0)
  {
    st[kStN] = st[kStCompact];  // what the compaction kept
    if (st[kStOff] | st[kStOff + 1] | st[kStOff + 2]) st[kStNbPoints] = st[kStCompact];  // Roll recounts the points when the grid moved (RollingGrid.cxx:136-137, 155)
  }
}

// ---- ClearOldPoints (RollingGrid.cxx:325-351) ----------------------------------------------------------------------
struct DecayPred
{
  const float4* pts;
  double now, threshold;
  __device__ bool operator()(int i) const
  {
    const float4 b = pts[2 * (size_t)i + 1];
    const unsigned label = (__float_as_uint(b.w) >> 24) & 0xffu;
    const double t = __hiloint2double(__float_as_int(b.y), __float_as_int(b.x));
    return !(!label && now - t > threshold);
  }
};
struct CopyEmit
{
  MapView src, dst;
  __device__ void operator()(int i, int at) const
  {
    dst.keys[at] = src.keys[i];
    dst.pts[2 * (size_t)at] = src.pts[2 * (size_t)i];
    dst.pts[2 * (size_t)at + 1] = src.pts[2 * (size_t)i + 1];
    dst.count[at] = src.count[i];
  }
};
// "Ordered" = 0: the keys ClearOldPoints erases, for the host's copy of the containers
struct ErasedPred
{
  DecayPred keep;
  __device__ bool operator()(int i) const { return !keep(i); }
};
struct KeyEmit
{
  const u64* keys;
  u64* out;
  __device__ void operator()(int i, int at) const { out[at] = keys[i]; }
};
__global__ void k_set_int(int* __restrict__ p, int v) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = v; }

}  // namespace

namespace lsa
{
// n_upper counts every point ever added; the exact number of voxels comes back with the state copy that follows each
// modification, and replaces the bound as soon as the last of those copies has landed
void tighten(lsa_device_grid* g)
{
  if (g->n_upper > 0 && hipEventQuery(g->ev_state) == hipSuccess) g->n_upper = std::min(g->n_upper, std::max(g->host_st[kStN], 0));
}

// a sub-map extraction (on the context's stream) reads the map and uses the grid's scratch: modifications come behind it
int after_submap(lsa_device_grid* g)
{
  G_HIP(hipStreamWaitEvent(g->stream, g->ev_sub, 0));
  g->ahead_phase = 0;  // a sub-map extracted ahead of time was of the map before this modification
  return LSA_OK;
}

int order_after_context(lsa_device_grid* g)
{
  G_HIP(hipEventRecord(g->ev_in, g->ctx->stream));
  G_HIP(hipStreamWaitEvent(g->stream, g->ev_in, 0));
  return LSA_OK;
}

GridParams params_of(const lsa_device_grid* g)
{
  GridParams p;
  p.grid_size = g->GridSize;
  p.resolution = (float)g->VoxelResolution;
  p.resolution_d = g->VoxelResolution;
  p.leaf = (float)g->LeafSize;
  p.leaf_d = g->LeafSize;
  p.sampling = g->Sampling;
  p.min_frames = g->MinFramesPerVoxel;
  return p;
}

int alloc_view(lsa_device_grid* g, MapView& v, int cap)
{
  G_HIP(hipMalloc((void**)&v.keys, (size_t)cap * sizeof(u64)));
  G_HIP(hipMalloc((void**)&v.pts, (size_t)cap * 2 * sizeof(float4)));
  G_HIP(hipMalloc((void**)&v.count, (size_t)cap * sizeof(unsigned)));
  return LSA_OK;
}
static void free_view(MapView& v)
{
  if (v.keys) (void)hipFree(v.keys);
  if (v.pts) (void)hipFree(v.pts);
  if (v.count) (void)hipFree(v.count);
  v = MapView{};
}
// an outgrown view while the grid lives: retired with its context (lsa_ctx.h: grave_dev), freed at the next frame's start
void retire_view(lsa_device_grid* g, MapView& v)
{
  retire_dev(g->ctx, v.keys);
  retire_dev(g->ctx, v.pts);
  retire_dev(g->ctx, v.count);
  v = MapView{};
}

// room for `want` voxels in both buffers of the map (contents kept) and for the chunk counters of a compaction over them
int ensure_map(lsa_device_grid* g, int want)
{
  if (want > g->cap)
  {
    const int cap = (int)std::min(std::max(2ll * want, 1ll << 19), kAddressable);  // 46 MB for both buffers: growth (a device-wide stall) is rare
    G_HIP(hipStreamSynchronize(g->stream));
    MapView nb[2];
    for (int b = 0; b < 2; ++b)
    {
      int rc = alloc_view(g, nb[b], cap);
      if (rc) return rc;
    }
    if (g->cap > 0)
    {
      const MapView& o = g->buf[g->cur];
      G_HIP(hipMemcpy(nb[0].keys, o.keys, (size_t)g->cap * sizeof(u64), hipMemcpyDeviceToDevice));
      G_HIP(hipMemcpy(nb[0].pts, o.pts, (size_t)g->cap * 2 * sizeof(float4), hipMemcpyDeviceToDevice));
      G_HIP(hipMemcpy(nb[0].count, o.count, (size_t)g->cap * sizeof(unsigned), hipMemcpyDeviceToDevice));
      retire_view(g, g->buf[0]);
      retire_view(g, g->buf[1]);
    }
    g->buf[0] = nb[0];
    g->buf[1] = nb[1];
    g->cur = 0;
    g->cap = cap;
    retire_dev(g->ctx, g->old_local);
    g->old_local = nullptr;
    G_HIP(hipMalloc((void**)&g->old_local, (size_t)cap * sizeof(int)));
  }
  const int nchunks = (std::max(g->cap, g->bcap) + 1023) / 1024 + 1;
  if (nchunks > g->chunk_cap)
  {
    retire_dev(g->ctx, g->chunks);
    g->chunks = nullptr;
    G_HIP(hipMalloc((void**)&g->chunks, (size_t)nchunks * sizeof(int)));
    g->chunk_cap = nchunks;
  }
  return LSA_OK;
}

// the host's copy of the state follows every modification (asynchronously)
int refresh_state(lsa_device_grid* g)
{
  G_HIP(hipMemcpyAsync(g->host_st, g->st, kStInts * sizeof(int), hipMemcpyDeviceToHost, g->stream));
  G_HIP(hipEventRecord(g->ev_state, g->stream));
  G_HIP(hipEventRecord(g->ev_out, g->stream));
  return LSA_OK;
}

// What Add, Roll and decay have in common.  In front of the kernels: behind the last extraction, room for `voxels_wanted`
// voxels, and ("Ordered" = 0) the last record replayed and room for the next one's `record_entries` keys ...
int begin_modification(lsa_device_grid* g, int voxels_wanted, size_t record_entries)
{
  ++g->version;
  int rc = after_submap(g);
  if (!rc) rc = ensure_map(g, voxels_wanted);
  if (!rc && !g->Ordered) rc = apply_record(g);
  if (!rc && !g->Ordered) rc = ensure_rec(g, record_entries);
  return rc;
}
// ... and behind them: ("Ordered" = 0) the record on its way to the host, then the state
int end_modification(lsa_device_grid* g, int record_kind, size_t entries)
{
  if (!g->Ordered)
  {
    const int rc = send_record(g, record_kind, entries);
    if (rc) return rc;
  }
  return refresh_state(g);
}

// ---- what lsa_pcd.hip needs of a grid (lsa_device_grid_io.h) ----
lsa_ctx* grid_context(lsa_device_grid* g) { return g->ctx; }
hipStream_t grid_stream(lsa_device_grid* g) { return g->stream; }
// A fresh grid with another grid's geometry, sampling mode and order: the values as `src` holds them, not put through the
// setters again (SetVoxelResolution snaps to the leaf size of the moment it is called at).  `dst` is emptied.
int grid_adopt_parameters(lsa_device_grid* dst, const lsa_device_grid* src)
{
  int rc = lsa_device_grid_reset(dst, nullptr);
  if (!rc) rc = lsa_device_grid_set(dst, "Ordered", src->Ordered ? 1. : 0.);
  if (rc) return rc;
  dst->GridSize = src->GridSize;
  dst->VoxelResolution = src->VoxelResolution;
  dst->LeafSize = src->LeafSize;
  dst->Sampling = src->Sampling;
  return lsa_device_grid_reset(dst, nullptr);  // (the grid's position, snapped to the resolution it has now)
}
}  // namespace lsa

// Roll (always a pass into the other buffer: the host does not know whether the grid moves)
static int roll(lsa_device_grid* g, bool use_box)
{
  hipStream_t st = g->stream;
  const GridParams p = params_of(g);
  hipLaunchKernelGGL(k_roll_decide, dim3(1), dim3(64), 0, st, p, g->st, use_box ? 1 : 0);
  const MapView src = g->buf[g->cur], dst = g->buf[1 - g->cur];
  RollPred pred{src.keys, g->st, g->GridSize};
  RollEmit emit{pred, src, dst};
  compact(g, pred, emit, g->st + kStN, std::max(g->n_upper, 1), g->st + kStN, false, false);
  hipLaunchKernelGGL(k_after_roll, dim3(1), dim3(64), 0, st, g->st);
  g->cur = 1 - g->cur;
  return LSA_OK;
}

extern "C" {

int lsa_device_grid_create(lsa_ctx* ctx, lsa_device_grid** out)
{
  if (!ctx || !out) return LSA_E_ARG;
  *out = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess) return LSA_E_HIP;
  lsa_device_grid* g = new lsa_device_grid;
  g->ctx = ctx;
  bool ok = hipMalloc((void**)&g->st, kStInts * sizeof(int)) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&g->host_st, kStInts * sizeof(int), hipHostMallocDefault) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&g->host_sub, sizeof(u64), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
  if (ok) *g->host_sub = 0;
  ok = ok && hipHostMalloc((void**)&g->host_ahead, 2 * sizeof(u64), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
  if (ok) g->host_ahead[0] = g->host_ahead[1] = 0;
  ok = ok && hipHostMalloc((void**)&g->rec_st, kStInts * sizeof(int), hipHostMallocDefault) == hipSuccess;
  {
    // The maps' kernels go on the context's LOOK-AHEAD stream (next frame's extraction, next ego-motion targets): a
    // process has four hardware queues, and the registration's stream, the look-ahead stream and the copy stream are
    // busy beside the insertions -- every further stream shares a queue with one of them, and when that one is the
    // ICP's the frame pays (one box, alternating runs: ego-motion phase 0.42 ms per frame with the maps on the
    // look-ahead stream, 0.60 with a stream per map, 0.83 with one new stream for all maps; 890 / 765 / 665 frames/s).
    // The order on that stream is the order of need: insertions (end of frame f), extraction of frame f + 2 (announced
    // during frame f + 1), targets of frame f + 2.
    // LSA_MAP_STREAM=own|shared: a stream per map / one more stream for all maps (the experiments above)
    const char* e = std::getenv("LSA_MAP_STREAM");
    const std::string mode = e ? e : "prefetch";
    int least = 0, greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (mode == "own") { ok = ok && hipStreamCreateWithPriority(&g->stream, hipStreamNonBlocking, least) == hipSuccess; g->own_stream = true; }
    else if (mode != "shared" && ctx->prefetch_stream) g->stream = ctx->prefetch_stream;
    else
    {
      if (!ctx->map_stream) ok = ok && hipStreamCreateWithPriority(&ctx->map_stream, hipStreamNonBlocking, least) == hipSuccess;
      g->stream = ctx->map_stream;
      if (ok) { ctx->map_stream_users++; g->shared_stream = true; }
    }
  }
  for (hipEvent_t* e : {&g->ev_state, &g->ev_in, &g->ev_out, &g->ev_sub, &g->ev_ahead, &g->ev_rec, &g->ev_order}) ok = ok && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
  if (!ok) { lsa_device_grid_destroy(g); return LSA_E_HIP; }
  *out = g;
  return lsa_device_grid_reset(g, nullptr);
}

void lsa_device_grid_destroy(lsa_device_grid* g)
{
  if (!g) return;
  (void)hipSetDevice(g->ctx->device);
  if (g->stream) (void)hipStreamSynchronize(g->stream);
  (void)hipStreamSynchronize(g->ctx->stream);  // a match may still read a sub-map: nothing of the grid is in use after this
  free_view(g->buf[0]); free_view(g->buf[1]); free_view(g->fresh);
  auto fr = [](void* p) { if (p) (void)hipFree(p); };
  fr(g->st); fr(g->batch); fr(g->bkeys); fr(g->skeys); fr(g->border); fr(g->sorder); fr(g->heads); fr(g->fresh_flag); fr(g->vrank); fr(g->chunks); fr(g->old_local);
  fr(g->oscan); fr(g->fscan); fr(g->scan_sums);
  fr(g->rec_dev); fr(g->order_dev); fr(g->perm);
  for (void* h : {(void*)g->rec_st, (void*)g->rec_host, (void*)g->order_host})
    if (h) (void)hipHostFree(h);
  if (g->host_st) (void)hipHostFree(g->host_st);
  if (g->host_sub) (void)hipHostFree(g->host_sub);
  if (g->host_ahead) (void)hipHostFree(g->host_ahead);
  for (hipEvent_t e : {g->ev_state, g->ev_in, g->ev_out, g->ev_sub, g->ev_ahead, g->ev_rec, g->ev_order})
    if (e) (void)hipEventDestroy(e);
  if (g->stream && g->own_stream) (void)hipStreamDestroy(g->stream);
  if (g->shared_stream && --g->ctx->map_stream_users == 0 && g->ctx->map_stream)
  {
    (void)hipStreamDestroy(g->ctx->map_stream);
    g->ctx->map_stream = nullptr;
  }
  delete g;
}

// RollingGrid::Reset (RollingGrid.cxx:40-48): the map is emptied, the grid is centred on `position` (snapped to the
// voxel resolution)
int lsa_device_grid_reset(lsa_device_grid* g, const float position[3])
{
  if (!g) return LSA_E_ARG;
  G_HIP(hipSetDevice(g->ctx->device));
  int h[kStInts] = {0};
  const float r = (float)g->VoxelResolution;
  for (int d = 0; d < 3; ++d)
  {
    const float v = std::floor((position ? position[d] : 0.f) / r) * r;
    std::memcpy(&h[kStPosX + d], &v, sizeof(float));
    h[kStTmp + d] = kBoxLoArmedS;
    h[kStTmp + 3 + d] = kBoxHiArmedS;
  }
  G_HIP(hipStreamSynchronize(g->stream));
  G_HIP(hipMemcpy(g->st, h, sizeof(h), hipMemcpyHostToDevice));
  std::memcpy(g->host_st, h, sizeof(h));
  ++g->version;
  g->n_upper = 0;
  g->submap_valid = false;
  return g->Ordered ? LSA_OK : forget_records(g);  // Reset goes through Clear (RollingGrid.cxx:40-48)
}

int lsa_device_grid_clear(lsa_device_grid* g)
{
  if (!g) return LSA_E_ARG;
  G_HIP(hipSetDevice(g->ctx->device));
  int rc = after_submap(g);
  if (rc) return rc;
  hipLaunchKernelGGL(k_set_int, dim3(1), dim3(64), 0, g->stream, g->st + kStN, 0);
  hipLaunchKernelGGL(k_set_int, dim3(1), dim3(64), 0, g->stream, g->st + kStNbPoints, 0);
  ++g->version;
  g->n_upper = 0;
  g->submap_valid = false;
  if (!g->Ordered) rc = forget_records(g);
  return rc ? rc : refresh_state(g);
}

static int readd_everything(lsa_device_grid* g, int ordered = -1)
{
  // prevMap = Get(); Clear(); Add(prevMap) -- and, for the "Ordered" setter, the new order between the Get and the Clear
  std::vector<lsa_point_t> all(std::max(g->n_upper, 1));
  const int n = g->n_upper > 0 ? lsa_device_grid_get(g, 0, all.data(), (int)all.size()) : 0;
  if (n < 0) return n;
  if (ordered >= 0)
  {
    if (!ordered)
    {
      g->shadow.Fresh();
      g->rec_kind = 0;  // (none: the grid was in key order)
      g->rec_voxels = 0;
      g->order_stale = true;
    }
    g->Ordered = ordered != 0;
  }
  int rc = lsa_device_grid_clear(g);
  if (rc) return rc;
  if (n > 0) return lsa_device_grid_add(g, all.data(), n, 0, -1., 1);
  return LSA_OK;
}

int lsa_device_grid_set(lsa_device_grid* g, const char* name, double value)
{
  if (!g || !name) return LSA_E_ARG;
  const std::string n(name);
  if (n == "LeafSize") { g->LeafSize = value; return LSA_OK; }
  if (n == "MinFramesPerVoxel") { g->MinFramesPerVoxel = (unsigned)value; return LSA_OK; }
  if (n == "Sampling") { g->Sampling = (int)value; return LSA_OK; }
  if (n == "DecayingThreshold") { g->DecayingThreshold = value; return LSA_OK; }
  if (n == "GlobalScans")
  {
    // (a test knob: which form an insertion takes is otherwise a matter of its size alone, lsa_grid_add.hip)
    if (value != 0. && value != 1. && value != 2.) return g->ctx->fail(LSA_E_ARG, "lsa_device_grid_set: GlobalScans is 0, 1 or 2");
    g->GlobalScans = (int)value;
    return LSA_OK;
  }
  if (n == "Ordered")
  {
    // RollingGrid::SetOrdered.  On an empty grid, from the first insertion on.  On a grid that holds points, the way the
    // geometry setters do it: the points, in the order they are handed out now, go back into the emptied grid (time -1,
    // not fixed, counts start again: a decaying map loses them at the next ClearOldPoints); to the reference's order,
    // into containers never used before.
    const int want = value != 0 ? 1 : 0;
    if ((want != 0) == g->Ordered) return LSA_OK;
    G_HIP(hipSetDevice(g->ctx->device));
    return readd_everything(g, want);
  }
  if (n == "GridSize")
  {
    // RollingGrid::SetGridSize (:59-70): the points are put back into the resized grid
    g->GridSize = (int)value;
    return readd_everything(g);
  }
  if (n == "VoxelResolution")
  {
    // RollingGrid::SetVoxelResolution (:73-88): a multiple of the leaf size; the grid position is snapped to it
    g->VoxelResolution = int(value / g->LeafSize) * g->LeafSize;
    G_HIP(hipSetDevice(g->ctx->device));
    G_HIP(hipStreamSynchronize(g->stream));
    int h[kStInts];
    G_HIP(hipMemcpy(h, g->st, sizeof(h), hipMemcpyDeviceToHost));
    const float r = (float)g->VoxelResolution;
    for (int d = 0; d < 3; ++d)
    {
      float v;
      std::memcpy(&v, &h[kStPosX + d], sizeof(float));
      v = std::floor(v / r) * r;
      std::memcpy(&h[kStPosX + d], &v, sizeof(float));
    }
    G_HIP(hipMemcpy(g->st, h, sizeof(h), hipMemcpyHostToDevice));
    return readd_everything(g);
  }
  return g->ctx->fail(LSA_E_ARG, "lsa_device_grid_set: unknown parameter " + n);
}

double lsa_device_grid_get_param(const lsa_device_grid* g, const char* name)
{
  if (!g || !name) return 0.;
  const std::string n(name);
  if (n == "LeafSize") return g->LeafSize;
  if (n == "MinFramesPerVoxel") return g->MinFramesPerVoxel;
  if (n == "Sampling") return g->Sampling;
  if (n == "DecayingThreshold") return g->DecayingThreshold;
  if (n == "GridSize") return g->GridSize;
  if (n == "VoxelResolution") return g->VoxelResolution;
  if (n == "Ordered") return g->Ordered ? 1. : 0.;
  if (n == "GlobalScans") return g->GlobalScans;
  if (n == "Voxels")
  {
    // the voxels the map holds, Get(false)'s size, as of the last modification that has completed on the device (waits for it)
    if (hipSetDevice(g->ctx->device) != hipSuccess || hipEventSynchronize(g->ev_state) != hipSuccess) return 0.;
    return std::max(g->host_st[kStN], 0);
  }
  return 0.;
}

// RollingGrid::Size() as of the last modification that has completed on the device (waits for it)
int lsa_device_grid_size(lsa_device_grid* g)
{
  if (!g) return LSA_E_ARG;
  if (hipSetDevice(g->ctx->device) != hipSuccess || hipEventSynchronize(g->ev_state) != hipSuccess) return LSA_E_HIP;
  // every modification has landed: the bound on the number of voxels is the number itself.  (tighten() alone seldom found the
  // event complete in the pipeline -- something had always just been enqueued behind it --, the bound then grew by every
  // keyframe's points and the map's buffers were "outgrown" and doubled every twenty keyframes: a stall of the maps' stream,
  // three device-wide copies and eight buffers to free at the next frame's start, 0.3-0.6 ms each time.)
  if (g->n_upper > 0) g->n_upper = std::min(g->n_upper, std::max(g->host_st[kStN], 0));
  return g->host_st[kStNbPoints];
}

int lsa_device_grid_roll(lsa_device_grid* g, const float mn[3], const float mx[3])
{
  if (!g || !mn || !mx) return LSA_E_ARG;
  G_HIP(hipSetDevice(g->ctx->device));
  int rc = begin_modification(g, std::max(g->n_upper, 1), 0);
  if (rc) return rc;
  int box[6];
  for (int d = 0; d < 3; ++d) { box[d] = f2os(mn[d]); box[3 + d] = f2os(mx[d]); }
  G_HIP(hipMemcpyAsync(g->st + kStTmp, box, sizeof(box), hipMemcpyHostToDevice, g->stream));
  G_HIP(hipStreamSynchronize(g->stream));
  rc = roll(g, true);
  return rc ? rc : end_modification(g, kRecRoll, 0);
}

int lsa_device_grid_clear_old_points(lsa_device_grid* g, double now)
{
  if (!g) return LSA_E_ARG;
  G_HIP(hipSetDevice(g->ctx->device));
  const int rc = begin_modification(g, std::max(g->n_upper, 1), (size_t)std::max(g->n_upper, 1));
  if (rc) return rc;
  const MapView src = g->buf[g->cur], dst = g->buf[1 - g->cur];
  const DecayPred keep{src.pts, now, g->DecayingThreshold};
  // "Ordered" = 0: the keys that go, for the shadow
  if (!g->Ordered) compact(g, ErasedPred{keep}, KeyEmit{src.keys, g->rec_dev}, g->st + kStN, std::max(g->n_upper, 1), g->st + kStRec);
  compact(g, keep, CopyEmit{src, dst}, g->st + kStN, std::max(g->n_upper, 1), g->st + kStN);
  g->cur = 1 - g->cur;
  return end_modification(g, kRecDecay, 0);  // (the erased keys follow when their number is known: apply_record)
}

}  // extern "C"
