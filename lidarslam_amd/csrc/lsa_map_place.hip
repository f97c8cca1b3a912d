// lsa_map_place.hip -- place recognition against the MAPS: the descriptor of the map as seen from a viewpoint, for many
// viewpoints at once, and the search of the last frame's descriptor among them.  The definition is
// lsa_scan_descriptor.h (map_coord, then the frame descriptor's text verbatim), which the host statement (host/lsa_place.cpp)
// compiles too; the kernels below decide only who computes what.
//   k_map_slice_boxes  a workgroup per slice of the point array: its xy box, once per map version
//   k_map_describe     a workgroup per (viewpoint, row of slices): the points of its slices binned into an LDS image of the
//                      cells by atomic max on ordered words (k_log_describe's coding), the non-empty words then merged into
//                      the viewpoint's zeroed image in global memory by integer atomic max.  Maxima commute: the image does
//                      not depend on the slicing, on the order or on which slices were passed over as out of reach
//   k_map_finish       a workgroup per viewpoint: words -> cell values, then a lane per sector for the column norms
// Offer and finish are lsa_place_image.h's, k_log_describe's own.  The query's slot is written by k_log_describe and the
// table searched by k_place_search (lsa_place_io.h).
// The source is "two float4 per point, n points": a device grid's own array (MapView::pts) or an uploaded lsa_point_t array.
// The table belongs to the context and is kept between calls; nothing is freed while work may be in flight (the graveyard).
#include <algorithm>
#include <cstring>
#include <vector>
#include "lsa_grid.h"
#include "lsa_place_image.h"
#include "lsa_place_io.h"

using namespace lsa;

namespace
{
constexpr int kThreads = 256;
constexpr int kDefaultSlice = 4096;   // points a slice, unless lsa_debug_set "map_describe_slice" says otherwise
constexpr int kTargetBlocks = 2048;   // workgroups a description aims at: rows of slices per viewpoint = kTargetBlocks / V

// up to three point arrays, cut into slices that are numbered through: source k has the slices first[k] .. first[k + 1] - 1
struct MapSources
{
  const float4* pts[3];
  int n[3];
  int first[4];
};
__device__ __forceinline__ void slice_range(const MapSources& m, int slice_size, int s, int* k, int* begin, int* end)
{
  int src = 0;
  while (src < 2 && s >= m.first[src + 1]) ++src;
  const long long b = (long long)(s - m.first[src]) * slice_size;
  *k = src;
  *begin = (int)b;
  *end = (int)min(b + slice_size, (long long)m.n[src]);
}

// A workgroup per slice: min / max of x and y over its points (fminf / fmaxf: a NaN takes no part; a slice of NaNs keeps the
// empty box, which is out of every reach).
__global__ __launch_bounds__(kThreads) void k_map_slice_boxes(MapSources m, int slice_size, float4* __restrict__ boxes)
{
  __shared__ float s_scr[4][kThreads / 64];
  int k, begin, end;
  slice_range(m, slice_size, blockIdx.x, &k, &begin, &end);
  const float4* __restrict__ pts = m.pts[k];
  float lox = FLT_MAX, loy = FLT_MAX, hix = -FLT_MAX, hiy = -FLT_MAX;
  for (int i = begin + (int)threadIdx.x; i < end; i += kThreads)
  {
    const float4 a = pts[2 * (size_t)i];
    lox = fminf(lox, a.x); hix = fmaxf(hix, a.x);
    loy = fminf(loy, a.y); hiy = fmaxf(hiy, a.y);
  }
  lox = block_reduce<kThreads / 64>(lox, OpMin(), s_scr[0]);
  loy = block_reduce<kThreads / 64>(loy, OpMin(), s_scr[1]);
  hix = block_reduce<kThreads / 64>(hix, OpMax(), s_scr[2]);
  hiy = block_reduce<kThreads / 64>(hiy, OpMax(), s_scr[3]);
  if (threadIdx.x == 0) boxes[blockIdx.x] = make_float4(lox, loy, hix, hiy);
}

// blockIdx.x: the viewpoint; blockIdx.y strides the slices.  Whether a slice is passed over depends on its box and the
// viewpoint alone, so the whole workgroup takes the same way; one that met no slice in reach leaves before the merge.
__global__ __launch_bounds__(kThreads) void k_map_describe(MapSources m, int slice_size, int slices, const float4* __restrict__ boxes /* nullptr: no slice is passed over */,
                                                           const double* __restrict__ viewpoints, unsigned* __restrict__ images, lsa_place_params_t p, double reach2)
{
  __shared__ unsigned s_img[kImageCells];
  const int cells = p.rings * p.sectors;  // <= kImageCells: the parameters were checked
  const double vx = viewpoints[3 * (size_t)blockIdx.x], vy = viewpoints[3 * (size_t)blockIdx.x + 1], vz = viewpoints[3 * (size_t)blockIdx.x + 2];
  for (int c = threadIdx.x; c < cells; c += kThreads) s_img[c] = 0u;
  __syncthreads();
  bool touched = false;
  for (int s = blockIdx.y; s < slices; s += gridDim.y)
  {
    if (boxes)
    {
      const float4 b = boxes[s];
      if (place::map_box_distance2(b.x, b.y, b.z, b.w, vx, vy) > reach2) continue;
    }
    touched = true;
    int k, begin, end;
    slice_range(m, slice_size, s, &k, &begin, &end);
    const float4* __restrict__ pts = m.pts[k];
    for (int i = begin + (int)threadIdx.x; i < end; i += kThreads)
    {
      const float4 a = pts[2 * (size_t)i];
      const float x = place::map_coord(a.x, vx), y = place::map_coord(a.y, vy), z = place::map_coord(a.z, vz);
      // out of reach (lsa_scan_descriptor.h: map_reach) before the square root and the angle; a NaN compares false and is cell_of's
      if ((double)x * (double)x + (double)y * (double)y > reach2) continue;
      image_offer(s_img, p, x, y, z);
    }
  }
  if (!touched) return;
  __syncthreads();
  unsigned* __restrict__ img = images + (size_t)blockIdx.x * (size_t)cells;
  for (int c = threadIdx.x; c < cells; c += kThreads)
  {
    const unsigned u = s_img[c];
    if (u) atomicMax(&img[c], u);
  }
}

// A workgroup per viewpoint: the merged image finished from global words into LDS floats.
__global__ __launch_bounds__(kThreads) void k_map_finish(const unsigned* __restrict__ images, float* __restrict__ table, int stride, lsa_place_params_t p)
{
  __shared__ float s_val[kImageCells];
  image_finish<kThreads>(images + (size_t)blockIdx.x * (size_t)(p.rings * p.sectors), s_val, table + (size_t)blockIdx.x * (size_t)stride, p);
}

struct SourceKey
{
  const void* grid = nullptr;
  unsigned long long version = 0;
  int n = 0;
  bool operator==(const SourceKey& o) const { return grid == o.grid && version == o.version && n == o.n; }
};
}  // namespace

namespace lsa
{
struct MapPlaceStore
{
  lsa_place_params_t params;
  bool valid = false;             // the table holds the descriptors of `viewpoints` under `params` of the sources `key`
  std::vector<double> viewpoints;
  int V = 0, stride = 0;
  SourceKey key[3];
  bool from_grids = false;
  bool query_valid = false;
  // the slices of the last description and their boxes
  int slice_size = 0, slices = 0;
  bool boxes_valid = false;
  SourceKey boxes_key[3];
  float4* boxes = nullptr;
  int boxes_cap = 0;
  float* table = nullptr;         // [V + 1][stride]
  size_t table_cap = 0;           // floats
  unsigned* images = nullptr;     // [V][cells]
  size_t images_cap = 0;          // words
  double* vp_dev = nullptr;
  size_t vp_cap = 0;              // doubles
  lsa_point_t* upload = nullptr;  // lsa_map_place_describe_points' copy of the caller's points
  size_t upload_cap = 0;          // points
  DescribeFrame* frame_dev = nullptr;
  DescribeFrame frame_host;
};

void map_place_destroy(lsa_ctx* ctx)
{
  MapPlaceStore* st = ctx->map_place;
  if (!st) return;
  for (void* p : {(void*)st->boxes, (void*)st->table, (void*)st->images, (void*)st->vp_dev, (void*)st->upload, (void*)st->frame_dev})
    if (p) (void)hipFree(p);
  delete st;
  ctx->map_place = nullptr;
}
}  // namespace lsa

namespace
{
// room for `count` elements in a device buffer of the store: half as much again, 64 at the least
template <typename T, typename N>
int room(lsa_ctx* ctx, T** buf, N* cap, size_t count) { return scratch_room<T>(ctx, buf, nullptr, cap, count, 64); }

int check_call(lsa_ctx* ctx, const char* who, const lsa_place_params_t* params, const double* viewpoints, int V)
{
  if (!ctx) return LSA_E_ARG;
  if (int rc = check_params(ctx, who, params)) return rc;
  if (!viewpoints || V < 1) return ctx->fail(LSA_E_ARG, std::string(who) + ": at least one viewpoint");
  for (size_t i = 0; i < 3 * (size_t)V; ++i)
    if (!(viewpoints[i] - viewpoints[i] == 0.)) return ctx->fail(LSA_E_ARG, std::string(who) + ": viewpoint " + std::to_string(i / 3) + " is not finite");
  return LSA_OK;
}

// The descriptors of `m` at the viewpoints into slots 0..V-1 of the table, enqueued on `stream`; the caller waits.
int describe(lsa_ctx* ctx, MapPlaceStore* st, const MapSources& src, const SourceKey key[3], const lsa_place_params_t& p, const double* viewpoints, int V, hipStream_t stream)
{
  st->valid = false;
  st->query_valid = false;
  const int cells = place::cells(p), stride = place::length(p);
  const int slice_size = ctx->map_describe_slice > 0 ? ctx->map_describe_slice : kDefaultSlice;
  MapSources m = src;
  m.first[0] = 0;
  for (int k = 0; k < 3; ++k)
  {
    const long long first = (long long)m.first[k] + ((long long)m.n[k] + slice_size - 1) / slice_size;
    if (first > 0x7fffffffLL) return ctx->fail(LSA_E_CAPACITY, "lsa_map_place: more slices than an int counts");
    m.first[k + 1] = (int)first;
  }
  const int slices = m.first[3];
  int rc = room(ctx, &st->table, &st->table_cap, ((size_t)V + 1) * (size_t)stride);
  if (!rc) rc = room(ctx, &st->images, &st->images_cap, (size_t)V * (size_t)cells);
  if (!rc) rc = room(ctx, &st->vp_dev, &st->vp_cap, 3 * (size_t)V);
  if (!rc) rc = room(ctx, &st->boxes, &st->boxes_cap, (size_t)std::max(slices, 1));
  if (rc) return rc;
  st->viewpoints.assign(viewpoints, viewpoints + 3 * (size_t)V);
  LSA_HIP(ctx, hipMemcpyAsync(st->vp_dev, st->viewpoints.data(), 3 * (size_t)V * sizeof(double), hipMemcpyHostToDevice, stream));
  LSA_HIP(ctx, hipMemsetAsync(st->images, 0, (size_t)V * (size_t)cells * sizeof(unsigned), stream));
  long long points = 0;
  for (int k = 0; k < 3; ++k) points += m.n[k];
  const bool same_map = st->boxes_valid && st->slice_size == slice_size && st->boxes_key[0] == key[0] && st->boxes_key[1] == key[1] && st->boxes_key[2] == key[2];
  if (slices > 0 && !(same_map && st->from_grids))
  {
    // (an uploaded array has no version to go by: its boxes are made every time)
    st->boxes_valid = false;
    ProfScope ps(ctx, "map_slice_boxes", (double)points * 32 + (double)slices * sizeof(float4), stream);
    hipLaunchKernelGGL(k_map_slice_boxes, dim3((unsigned)slices), dim3(kThreads), 0, stream, m, slice_size, st->boxes);
    LSA_HIP(ctx, hipGetLastError());
  }
  st->slice_size = slice_size;
  st->slices = slices;
  for (int k = 0; k < 3; ++k) st->boxes_key[k] = key[k];
  st->boxes_valid = true;
  if (slices > 0)
  {
    const int rows = std::min(std::min(slices, 65535), std::max(1, (kTargetBlocks + V - 1) / V));
    ProfScope ps(ctx, "map_describe", (double)points * 32 * V + (double)V * cells * 4, stream);
    hipLaunchKernelGGL(k_map_describe, dim3((unsigned)V, (unsigned)rows), dim3(kThreads), 0, stream, m, slice_size, slices, ctx->map_describe_cull ? st->boxes : nullptr,
                       st->vp_dev, st->images, p, place::map_reach(p) * place::map_reach(p));
    LSA_HIP(ctx, hipGetLastError());
  }
  {
    ProfScope ps(ctx, "map_finish", (double)V * (cells + stride) * 4, stream);
    hipLaunchKernelGGL(k_map_finish, dim3((unsigned)V), dim3(kThreads), 0, stream, st->images, st->table, stride, p);
    LSA_HIP(ctx, hipGetLastError());
  }
  LSA_HIP(ctx, hipStreamSynchronize(stream));
  st->params = p;
  st->V = V;
  st->stride = stride;
  for (int k = 0; k < 3; ++k) st->key[k] = key[k];
  st->valid = true;
  return LSA_OK;
}

MapPlaceStore* store_of(lsa_ctx* ctx)
{
  if (!ctx->map_place) ctx->map_place = new MapPlaceStore;
  return ctx->map_place;
}
}  // namespace

extern "C" {

int lsa_map_place_describe_points(lsa_ctx* ctx, const lsa_place_params_t* params, const lsa_point_t* pts, int n, const double* viewpoints, int V)
{
  const char* who = "lsa_map_place_describe_points";
  int rc = check_call(ctx, who, params, viewpoints, V);
  if (rc) return rc;
  if (n < 0 || (n > 0 && !pts)) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  MapPlaceStore* st = store_of(ctx);
  rc = room(ctx, &st->upload, &st->upload_cap, (size_t)std::max(n, 1));
  if (rc) return rc;
  if (n > 0) LSA_HIP(ctx, hipMemcpyAsync(st->upload, pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyHostToDevice, ctx->stream));
  MapSources m = {};
  m.pts[0] = reinterpret_cast<const float4*>(st->upload);
  m.n[0] = n;
  SourceKey key[3];
  key[0].n = n;
  st->from_grids = false;
  rc = describe(ctx, st, m, key, *params, viewpoints, V, ctx->stream);
  return rc ? rc : V;
}

int lsa_map_place_describe_grids(lsa_ctx* ctx, lsa_device_grid* const grids[3], const lsa_place_params_t* params, const double* viewpoints, int V)
{
  const char* who = "lsa_map_place_describe_grids";
  int rc = check_call(ctx, who, params, viewpoints, V);
  if (rc) return rc;
  if (!grids) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  lsa_device_grid* used[3] = {nullptr, nullptr, nullptr};
  for (int k = 0; k < 3; ++k)
    if (((params->type_mask >> k) & 1u) && grids[k])
    {
      if (grids[k]->ctx != ctx) return ctx->fail(LSA_E_ARG, std::string(who) + ": a grid of another context");
      used[k] = grids[k];
    }
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  MapPlaceStore* st = store_of(ctx);
  // what the grids hold as of their last modification, which is waited for (lsa_device_grid_size does the same)
  MapSources m = {};
  SourceKey key[3];
  hipStream_t stream = nullptr;
  for (int k = 0; k < 3; ++k)
  {
    lsa_device_grid* g = used[k];
    if (!g) continue;
    LSA_HIP(ctx, hipEventSynchronize(g->ev_state));
    const int n = g->n_upper > 0 ? std::max(g->host_st[kStN], 0) : 0;
    m.pts[k] = g->buf[g->cur].pts;
    m.n[k] = m.pts[k] ? n : 0;
    key[k].grid = g;
    key[k].version = g->version;
    key[k].n = m.n[k];
    if (!stream) stream = g->stream;
  }
  if (st->valid && st->from_grids && st->V == V && same_params(st->params, *params) && st->key[0] == key[0] && st->key[1] == key[1] &&
      st->key[2] == key[2] && std::memcmp(st->viewpoints.data(), viewpoints, 3 * (size_t)V * sizeof(double)) == 0)
    return 0;
  if (!stream) stream = ctx->stream;
  // on the maps' stream, behind every used grid's last modification (ev_out), as an extraction of theirs
  for (int k = 0; k < 3; ++k)
    if (used[k] && used[k]->stream != stream) LSA_HIP(ctx, hipStreamWaitEvent(stream, used[k]->ev_out, 0));
  st->from_grids = true;
  rc = describe(ctx, st, m, key, *params, viewpoints, V, stream);
  return rc ? rc : V;
}

int lsa_map_place_descriptors(lsa_ctx* ctx, int first, int last, float* out)
{
  if (!ctx) return LSA_E_ARG;
  MapPlaceStore* st = ctx->map_place;
  if (!st || !st->valid) return ctx->fail(LSA_E_STATE, "lsa_map_place_descriptors: no table (lsa_map_place_describe_points / _grids)");
  if (!out || first < 0 || last < first || last > st->V) return ctx->fail(LSA_E_ARG, "lsa_map_place_descriptors: bad argument");
  if (last == st->V && !st->query_valid) return ctx->fail(LSA_E_STATE, "lsa_map_place_descriptors: the query's slot has not been described (lsa_map_place_search)");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipMemcpyAsync(out, st->table + (size_t)first * st->stride, (size_t)(last - first + 1) * st->stride * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

int lsa_map_place_search(lsa_ctx* ctx, const lsa_place_params_t* params, int set, float* distance_out, int32_t* shift_out)
{
  const char* who = "lsa_map_place_search";
  if (!ctx) return LSA_E_ARG;
  if (int rc = check_params(ctx, who, params)) return rc;
  if (set < 0 || set > 2 || !distance_out || !shift_out) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  MapPlaceStore* st = ctx->map_place;
  if (!st || !st->valid) return ctx->fail(LSA_E_STATE, std::string(who) + ": no table (lsa_map_place_describe_points / _grids)");
  if (!same_params(st->params, *params)) return ctx->fail(LSA_E_STATE, std::string(who) + ": the table was described under other parameters");
  DescribeFrame f;
  long long points = 0;
  for (int k = 0; k < 3; ++k)
  {
    const bool use = (params->type_mask >> k) & 1u;
    f.pts[k] = reinterpret_cast<const float4*>(ctx->kp[set][k]);
    f.n[k] = use && f.pts[k] ? std::max(ctx->kp_n[set][k], 0) : 0;
    points += f.n[k];
  }
  f.slot = st->V;
  if (points == 0) return ctx->fail(LSA_E_STATE, std::string(who) + ": the keypoint set is empty");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const int V = st->V;
  if (!st->frame_dev) LSA_HIP(ctx, hipMalloc((void**)&st->frame_dev, sizeof(DescribeFrame)));
  st->query_valid = false;
  st->frame_host = f;
  LSA_HIP(ctx, hipMemcpyAsync(st->frame_dev, &st->frame_host, sizeof(DescribeFrame), hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "log_describe", (double)points * 32 + (double)st->stride * 4);
    place_describe_launch(st->frame_dev, 1, st->table, st->stride, st->params, ctx->stream);
  }
  LSA_HIP(ctx, hipGetLastError());
  const int rc = place_search_one(ctx, st->table, (long long)V + 1, 0, st->stride, st->params, V, 0, V, distance_out, shift_out);
  if (rc) return rc;
  st->query_valid = true;
  return LSA_OK;
}

int lsa_map_place_viewpoints(const lsa_ctx* ctx) { return ctx && ctx->map_place && ctx->map_place->valid ? ctx->map_place->V : 0; }

int lsa_map_place_slices(lsa_ctx* ctx, float* boxes, int capacity)
{
  if (!ctx) return LSA_E_ARG;
  MapPlaceStore* st = ctx->map_place;
  if (!st || !st->valid) return ctx->fail(LSA_E_STATE, "lsa_map_place_slices: no table (lsa_map_place_describe_points / _grids)");
  if (boxes)
  {
    if (capacity < st->slices) return ctx->fail(LSA_E_CAPACITY, "lsa_map_place_slices: room for " + std::to_string(capacity) + " of " + std::to_string(st->slices) + " boxes");
    LSA_HIP(ctx, hipSetDevice(ctx->device));
    if (st->slices > 0) LSA_HIP(ctx, hipMemcpy(boxes, st->boxes, (size_t)st->slices * sizeof(float4), hipMemcpyDeviceToHost));
  }
  return st->slices;
}

}  // extern "C"
