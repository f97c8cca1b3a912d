// lsa_dense_grid.hip -- the floor plan of the dense map: elevation and a 2-D occupancy grid (DESIGN.md 3.14 "The floor plan";
// the host statement, held byte for byte, is DenseMapHost.grid in lidarslam_amd/_dense_map.py).  Not on the frame path,
// nothing stored, read-only on the table: rasters of one call
//   k_dense_grid_bounds    (no window) the box of the kept voxels' cells
//   k_dense_grid_columns   every kept voxel: atomicMin of its z code into its cell of the extent widened by the radius
//   k_dense_grid_rows / _ground   one thread a cell: the smallest code of the neighbourhood, along the row, then along the column
//   k_dense_grid_band      every kept voxel against the ground of its cell: atomicAdd on a count, atomicMax on the top code
//   k_dense_grid_classify  one thread a cell: the 20-byte record and the state
#include <cmath>
#include <cstring>
#include <new>
#include <vector>
#include "lsa_dense_table.h"
#include "lsa_device_grid_io.h"
#include "lsa_wave.h"
#include "host/lsa_occupancy.h"

using namespace lsa;
using namespace lsa::dense;

namespace
{
// Rasters of one call, all in unsigned words.  Floats are folded as their ordered codes (f2ou), under which atomicMin and
// atomicMax give the host's answer in any order; counts add up.  The three voxel passes run over the table's slots under Keep --
// the lines a compacted list would send them to anyway, without the wait for its count.  The column raster is the extent
// widened by the radius on every side, so that the ground of a cell at the edge sees the columns outside.
struct Grid
{
  int cell_leaves, radius;
  int cx0, cy0, width, height;  // the extent
  double min_height, max_height;
  unsigned min_obstacle;
  Keep keep;
  unsigned* col;     // [(height + 2 radius) * (width + 2 radius)] the smallest z code of a column, armed ~0u
  unsigned* rows;    // [(height + 2 radius) * width] the minimum of 2 radius + 1 columns of a row
  unsigned* ground;  // [height * width]
  unsigned* floor;   // [height * width], then as many obstacle counts, then as many top codes (armed 0)
};
constexpr unsigned kNoCode = ~0u;

// floor division by a positive b
__device__ __forceinline__ int floor_div(int a, int b)
{
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ void cell_of(u64 key, int cell_leaves, int& cx, int& cy)
{
  cx = floor_div((int)key_index(key, 0), cell_leaves);
  cy = floor_div((int)key_index(key, 1), cell_leaves);
}

// launch 1 (no window): the box of the kept voxels' cells, lo x, lo y, hi x, hi y; four atomics at most a workgroup
constexpr unsigned kGridBoundsBlocks = 256;
__global__ __launch_bounds__(256) void k_dense_grid_bounds(Table t, Keep keep, int cell_leaves, unsigned turns, int* __restrict__ box)
{
  int lx = INT32_MAX, ly = INT32_MAX, hx = INT32_MIN, hy = INT32_MIN;
  // `turns` slots a thread, a whole grid apart: the launch has kGridBoundsBlocks workgroups at most, whatever the capacity
  for (unsigned turn = 0; turn < turns; ++turn)
  {
    const size_t i = ((size_t)turn * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x;
    if (i > (size_t)t.mask) break;
    const Slot& S = t.slots[i];
    if (!keep(S, (unsigned)i)) continue;
    int cx, cy;
    cell_of(S.key, cell_leaves, cx, cy);
    lx = min(lx, cx); ly = min(ly, cy); hx = max(hx, cx); hy = max(hy, cy);
  }
  // (every thread of the workgroup is here: nobody has left)
  __shared__ int scratch[4][4];
  lx = block_reduce<4>(lx, OpMin(), scratch[0]); ly = block_reduce<4>(ly, OpMin(), scratch[1]);
  hx = block_reduce<4>(hx, OpMax(), scratch[2]); hy = block_reduce<4>(hy, OpMax(), scratch[3]);
  // (one thread a slot and four atomics a wavefront -- 32 768 wavefronts of a table of 2^21 slots aiming at the same four
  //  words -- took 1.49 ms, and 0.21 ms with the reads below alone: the wavefronts in flight at the start all find the
  //  words armed.  So the workgroups are few and send one box each, and a word that already covers it is read and left
  //  alone: min and max only ever move one way, so a stale read costs an atomic that changes nothing, never a missed one)
  if (threadIdx.x == 0 && lx <= hx)
  {
    if (__hip_atomic_load(&box[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > lx) atomicMin(&box[0], lx);
    if (__hip_atomic_load(&box[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > ly) atomicMin(&box[1], ly);
    if (__hip_atomic_load(&box[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < hx) atomicMax(&box[2], hx);
    if (__hip_atomic_load(&box[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < hy) atomicMax(&box[3], hy);
  }
}

// launch 2: every kept voxel of the widened extent folds its z into its column
__global__ __launch_bounds__(256) void k_dense_grid_columns(Table t, const Grid g)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > t.mask) return;
  const Slot& S = t.slots[i];
  if (!g.keep(S, i)) return;
  int cx, cy;
  cell_of(S.key, g.cell_leaves, cx, cy);
  const int ex = cx - (g.cx0 - g.radius), ey = cy - (g.cy0 - g.radius);
  const int ew = g.width + 2 * g.radius, eh = g.height + 2 * g.radius;
  if (ex < 0 || ex >= ew || ey < 0 || ey >= eh) return;
  // (reading the word first, to spare the atomic of a voxel that cannot lower it, was measured and not kept: the atomic then
  //  waits for the read, where without it nothing is waited for -- 77 us against 39 us at 524 288 slots, no gain at 2 097 152)
  atomicMin(&g.col[(size_t)ey * (size_t)ew + (size_t)ex], f2ou(S.a.z));
}

// launches 3 and 4, one thread a cell: min by code is exact and associative, so the (2 radius + 1)^2 neighbourhood is a run
// along the row, then a run along the column
__global__ __launch_bounds__(256) void k_dense_grid_rows(const Grid g)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t w = (size_t)g.width, ew = w + 2 * (size_t)g.radius, eh = (size_t)g.height + 2 * (size_t)g.radius;
  if (i >= eh * w) return;
  const unsigned* from = g.col + (i / w) * ew + i % w;
  unsigned v = kNoCode;
  for (int d = 0; d <= 2 * g.radius; ++d) v = min(v, from[d]);
  g.rows[i] = v;
}
__global__ __launch_bounds__(256) void k_dense_grid_ground(const Grid g)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t w = (size_t)g.width;
  if (i >= (size_t)g.height * w) return;
  unsigned v = kNoCode;
  for (int d = 0; d <= 2 * g.radius; ++d) v = min(v, g.rows[i + (size_t)d * w]);
  g.ground[i] = v;
}

// launch 5: every kept voxel of the extent against the ground of its cell
__global__ __launch_bounds__(256) void k_dense_grid_band(Table t, const Grid g)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > t.mask) return;
  const Slot& S = t.slots[i];
  if (!g.keep(S, i)) return;
  int cx, cy;
  cell_of(S.key, g.cell_leaves, cx, cy);
  const int x = cx - g.cx0, y = cy - g.cy0;
  if (x < 0 || x >= g.width || y < 0 || y >= g.height) return;
  const size_t cells = (size_t)g.width * (size_t)g.height, at = (size_t)y * (size_t)g.width + (size_t)x;
  const unsigned low = g.ground[at];
  if (low == kNoCode) return;  // (never: the voxel's own column is in the neighbourhood)
  const float z = S.a.z;
  const double h = (double)z - (double)ou2f(low);
  if (h <= g.min_height) atomicAdd(&g.floor[at], 1u);
  else if (h <= g.max_height)
  {
    atomicAdd(&g.floor[cells + at], 1u);
    atomicMax(&g.floor[2 * cells + at], f2ou(z));
  }
}

// launch 6, one thread a cell: the record and the state
__global__ __launch_bounds__(256) void k_dense_grid_classify(const Grid g, unsigned* __restrict__ out, signed char* __restrict__ state)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t w = (size_t)g.width, cells = w * (size_t)g.height;
  if (i >= cells) return;
  const size_t ew = w + 2 * (size_t)g.radius;
  const unsigned elevation = g.col[(i / w + (size_t)g.radius) * ew + i % w + (size_t)g.radius];
  const unsigned low = g.ground[i], floor_voxels = g.floor[i], obstacle_voxels = g.floor[cells + i], top = g.floor[2 * cells + i];
  unsigned* o = out + 5 * i;
  o[0] = elevation != kNoCode ? __builtin_bit_cast(unsigned, ou2f(elevation)) : kQuietNaN;
  o[1] = low != kNoCode ? __builtin_bit_cast(unsigned, ou2f(low)) : kQuietNaN;
  o[2] = top != 0u ? __builtin_bit_cast(unsigned, ou2f(top)) : kQuietNaN;
  o[3] = floor_voxels;
  o[4] = obstacle_voxels;
  state[i] = obstacle_voxels >= g.min_obstacle ? (signed char)100 : (floor_voxels >= 1u ? (signed char)0 : (signed char)-1);
}

// where the last grid_raster left its records and states
struct GridOut
{
  const lsa_dense_cell_t* cells = nullptr;
  const signed char* state = nullptr;
};

// The floor plan of the voxels that pass: *info, and with want_cells the records and states of its cells on the device
// (*out), enqueued, not waited for.  Returns width * height.  A refusal comes before anything is waited for or allocated.
long long grid_raster(lsa_dense_map* dm, const lsa_dense_grid_params_t* p, lsa_dense_grid_info_t* info, bool want_cells, GridOut* out, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  if (p->cell_leaves < 1 || p->cell_leaves > 64) return ctx->fail(LSA_E_ARG, std::string(who) + ": cell_leaves between 1 and 64");
  if (p->ground_radius < 0 || p->ground_radius > 16) return ctx->fail(LSA_E_ARG, std::string(who) + ": ground_radius between 0 and 16 cells");
  if (!(std::isfinite(p->min_height) && std::isfinite(p->max_height) && p->min_height >= 0. && p->min_height < p->max_height))
    return ctx->fail(LSA_E_ARG, std::string(who) + ": 0 <= min_height < max_height, both finite");
  if (p->min_obstacle_voxels < 1) return ctx->fail(LSA_E_ARG, std::string(who) + ": min_obstacle_voxels >= 1");
  if (p->use_window)
  {
    const double* w = p->window;
    if (!(std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]) && std::isfinite(w[3]) && w[0] <= w[2] && w[1] <= w[3]))
      return ctx->fail(LSA_E_ARG, std::string(who) + ": window = (x_min, y_min, x_max, y_max), finite, x_min <= x_max, y_min <= y_max");
  }
  if (const int rc = settle(dm, who)) return rc;
  const int cl = p->cell_leaves, r = p->ground_radius;
  std::memset(info, 0, sizeof(*info));
  info->resolution = (double)cl * dm->leaf;
  const bool voxels = dm->slots && occupied_bound(dm) > 0;  // exact after settle
  const Keep keep = keep_of(dm, p->min_frames, p->max_miss_ratio);
  const dim3 over_slots((dm->capacity + 255u) / 256u);
  long long lo[2], hi[2];  // cells
  if (p->use_window)
  {
    for (int a = 0; a < 2; ++a)
    {
      // the two IEEE operations of the keys; a window wholly outside the index range has no cell, any other is clamped to it
      double i0 = std::floor(p->window[a] / dm->leaf), i1 = std::floor(p->window[2 + a] / dm->leaf);
      if (i1 < -kIndexRange || i0 >= kIndexRange) return 0;
      i0 = std::min(std::max(i0, -kIndexRange), kIndexRange - 1.);
      i1 = std::min(std::max(i1, -kIndexRange), kIndexRange - 1.);
      const long long v0 = (long long)i0, v1 = (long long)i1;
      lo[a] = v0 >= 0 ? v0 / cl : -((-v0 + cl - 1) / cl);  // floor division
      hi[a] = v1 >= 0 ? v1 / cl : -((-v1 + cl - 1) / cl);
    }
  }
  else
  {
    if (!voxels) return 0;
    if (!dm->grid_box)
    {
      if (hipMalloc((void**)&dm->grid_box, 4 * sizeof(int)) != hipSuccess)
      {
        (void)hipGetLastError();
        dm->grid_box = nullptr;
        return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory");
      }
    }
    static const int armed[4] = {INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN};
    int box[4];
    LSA_HIP(ctx, hipMemcpyAsync(dm->grid_box, armed, sizeof(armed), hipMemcpyHostToDevice, dm->stream));
    {
      ProfScope ps(ctx, "dense_grid_bounds", (double)dm->capacity * 64, dm->stream);
      const unsigned blocks = std::min(over_slots.x, kGridBoundsBlocks), turns = (dm->capacity + blocks * 256u - 1u) / (blocks * 256u);
      hipLaunchKernelGGL(k_dense_grid_bounds, dim3(blocks), dim3(256), 0, dm->stream, table_of(dm), keep, cl, turns, dm->grid_box);
    }
    LSA_HIP(ctx, hipGetLastError());
    LSA_HIP(ctx, hipMemcpyAsync(box, dm->grid_box, sizeof(box), hipMemcpyDeviceToHost, dm->stream));
    LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
    if (box[0] > box[2]) return 0;  // no voxel passes
    lo[0] = box[0]; lo[1] = box[1]; hi[0] = box[2]; hi[1] = box[3];
  }
  const long long W = hi[0] - lo[0] + 1, H = hi[1] - lo[1] + 1, cells = W * H;  // each at most 2^21
  if (cells > dm->grid_max_cells)
    return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": a grid of " + std::to_string(W) + " x " + std::to_string(H) + " cells is over GridMaxCells = " +
                                         std::to_string(dm->grid_max_cells) + "; ask for a window");
  info->cx0 = (int)lo[0];
  info->cy0 = (int)lo[1];
  info->width = (int)W;
  info->height = (int)H;
  info->origin_x = (double)(lo[0] * cl) * dm->leaf;
  info->origin_y = (double)(lo[1] * cl) * dm->leaf;
  if (!want_cells) return cells;
  // the rasters: col, rows, ground, floor / obstacle / top, the records (5 words a cell), the states (a byte a cell)
  const size_t n = (size_t)cells, ew = (size_t)W + 2 * (size_t)r, eh = (size_t)H + 2 * (size_t)r;
  const size_t words = eh * ew + eh * (size_t)W + n + 3 * n + 5 * n, bytes = words * sizeof(unsigned) + n;
  if (const int rc = room(dm, {{(void**)&dm->grid_scratch, 1}}, &dm->grid_scratch_cap, bytes, 4, who, "rasters", "; ask for a smaller window")) return rc;
  Grid g{};
  g.cell_leaves = cl;
  g.radius = r;
  g.cx0 = info->cx0; g.cy0 = info->cy0; g.width = info->width; g.height = info->height;
  g.min_height = p->min_height;
  g.max_height = p->max_height;
  g.min_obstacle = (unsigned)p->min_obstacle_voxels;
  g.keep = keep;
  g.col = reinterpret_cast<unsigned*>(dm->grid_scratch);
  g.rows = g.col + eh * ew;
  g.ground = g.rows + eh * (size_t)W;
  g.floor = g.ground + n;
  unsigned* records = g.floor + 3 * n;
  signed char* state = reinterpret_cast<signed char*>(records + 5 * n);
  LSA_HIP(ctx, hipMemsetAsync(g.col, 0xff, eh * ew * sizeof(unsigned), dm->stream));
  LSA_HIP(ctx, hipMemsetAsync(g.floor, 0, 3 * n * sizeof(unsigned), dm->stream));
  const auto blocks = [](size_t threads) { return dim3((unsigned)((threads + 255) / 256)); };
  if (voxels)
  {
    // per slot its 64-byte line; per voxel of the extent a 4-byte word
    ProfScope ps(ctx, "dense_grid_columns", (double)dm->capacity * 64 + (double)dm->known * 4, dm->stream);
    hipLaunchKernelGGL(k_dense_grid_columns, over_slots, dim3(256), 0, dm->stream, table_of(dm), g);
  }
  {
    ProfScope ps(ctx, "dense_grid_ground", (double)(eh * ew + 2 * eh * (size_t)W + n) * 4, dm->stream);
    hipLaunchKernelGGL(k_dense_grid_rows, blocks(eh * (size_t)W), dim3(256), 0, dm->stream, g);
    hipLaunchKernelGGL(k_dense_grid_ground, blocks(n), dim3(256), 0, dm->stream, g);
  }
  if (voxels)
  {
    // per slot its line; per voxel of the extent the ground word and one or two counted words
    ProfScope ps(ctx, "dense_grid_band", (double)dm->capacity * 64 + (double)dm->known * 12, dm->stream);
    hipLaunchKernelGGL(k_dense_grid_band, over_slots, dim3(256), 0, dm->stream, table_of(dm), g);
  }
  {
    ProfScope ps(ctx, "dense_grid_classify", (double)n * (5 * 4 + 21), dm->stream);
    hipLaunchKernelGGL(k_dense_grid_classify, blocks(n), dim3(256), 0, dm->stream, g, records, state);
  }
  LSA_HIP(ctx, hipGetLastError());
  out->cells = reinterpret_cast<const lsa_dense_cell_t*>(records);
  out->state = state;
  return cells;
}
}  // namespace

extern "C" {

long long lsa_dense_map_get_grid(lsa_dense_map* dm, const lsa_dense_grid_params_t* params, lsa_dense_grid_info_t* info, lsa_dense_cell_t* cells, int8_t* state,
                                 long long capacity)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_get_grid";
  if (!params || !info || capacity < 0) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  const double t0 = now_seconds();
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const bool want = capacity > 0 && (cells || state);  // nothing to write: the extent alone
  GridOut out;
  const long long n = grid_raster(dm, params, info, want, &out, who);
  if (n <= 0) return n;
  if (want)
  {
    const size_t take = (size_t)std::min(n, capacity);
    if (cells) LSA_HIP(ctx, hipMemcpyAsync(cells, out.cells, take * sizeof(lsa_dense_cell_t), hipMemcpyDeviceToHost, dm->stream));
    if (state) LSA_HIP(ctx, hipMemcpyAsync(state, out.state, take, hipMemcpyDeviceToHost, dm->stream));
    LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  }
  dm->grid_seconds = now_seconds() - t0;
  return n;
}

long long lsa_dense_map_save_grid(lsa_dense_map* dm, const lsa_dense_grid_params_t* params, const char* prefix)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_save_grid";
  if (!params || !prefix) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  try
  {
    LSA_HIP(ctx, hipSetDevice(ctx->device));
    lsa_dense_grid_info_t info;
    GridOut out;
    const long long n = grid_raster(dm, params, &info, true, &out, who);
    if (n <= 0) return n;  // a grid without cells is not saved
    std::vector<int8_t> state((size_t)n);
    LSA_HIP(ctx, hipMemcpyAsync(state.data(), out.state, (size_t)n, hipMemcpyDeviceToHost, dm->stream));
    LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
    std::string err;
    const long long written = occupancy::write(prefix, info, state.data(), err);
    return written < 0 ? ctx->fail((int)written, std::string(who) + ": " + err) : written;
  }
  catch (const std::bad_alloc&) { return ctx->fail(LSA_E_CAPACITY, std::string(prefix) + ": not enough host memory"); }
}

}  // extern "C"
