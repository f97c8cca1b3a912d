// lsa_dense_table.h -- what the units of the dense map share (lsa_dense_map.hip: the table, its insertions and exports;
// lsa_dense_cast.hip: rays through it): the slot, the table and its look-ups, the export's predicate, the move of a frame
// point to the world, the walk of a ray through the voxels, and the map's host object.  Internal: device code, HIP units only.
#pragma once
#include <cmath>
#include <cstdint>
#include <deque>
#include <string>
#include <utility>
#include "lsa_ctx.h"
#include "lsa_device_math.h"
#include "lsa_wave.h"

namespace lsa
{
typedef unsigned long long u64;  // (as lsa_compact.h)
namespace dense
{
constexpr u64 kOccupied = 1ull << 63;
constexpr double kIndexRange = 1048576.;  // 2^20: indices in [-2^20, 2^20)
constexpr unsigned kMinCapacity = 64, kMaxCapacity = 1u << 30;
constexpr size_t kDefaultMaxBytes = (size_t)16 << 30;
constexpr double kMaxRangeLeaves = 4096.;  // "CarveRange" / leaf and a cast's max_range / leaf at most

struct alignas(64) Slot
{
  u64 key;
  u64 cand;
  float4 a, b;  // the LidarPoint: x y z w | time, intensity, laser / device / label
  unsigned count, frames;
  int first, last;
};
static_assert(sizeof(Slot) == 64, "a slot is one 64-byte record");

struct Table
{
  Slot* slots;
  int* source;    // [capacity] the ordinal of the call whose point the slot holds
  unsigned* miss; // [2 * capacity] misses, then miss-frame words; null in a map never carved
  unsigned mask;  // capacity - 1
  int stress;     // "ProbeStress": every key's home slot is 0
};
// device words of a map: [0] occupied slots, [1] error (a probe sequence ran out), [2] points skipped, [3] voxels the
// re-projection in flight dropped, [4] rays carved, [5] rays cast (lsa_dense_cast.hip), [6..9] the labels of the compare in flight
enum { kStatOccupied = 0, kStatError = 1, kStatSkipped = 2, kStatDropped = 3, kStatRays = 4, kStatCastRays = 5, kStatLabels = 6, kStatWords = 10 };

// the order-preserving code of an intensity: f2ou, and 0 -- below -inf -- for a NaN
__device__ __forceinline__ unsigned intensity_code(float v) { return v == v ? f2ou(v) : 0u; }

__device__ __forceinline__ bool voxel_key(const float4& a, double leaf, u64& key)
{
  if (!(__builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z))) return false;
  const double ix = __builtin_floor((double)a.x / leaf), iy = __builtin_floor((double)a.y / leaf), iz = __builtin_floor((double)a.z / leaf);
  if (!(ix >= -kIndexRange && ix < kIndexRange && iy >= -kIndexRange && iy < kIndexRange && iz >= -kIndexRange && iz < kIndexRange)) return false;
  key = ((u64)((long long)iz + 1048576ll) << 42) | ((u64)((long long)iy + 1048576ll) << 21) | (u64)((long long)ix + 1048576ll);
  return true;
}

__device__ __forceinline__ unsigned home_slot(const Table& t, u64 key)
{
  if (t.stress) return 0u;
  key ^= key >> 33; key *= 0xff51afd7ed558ccdull;
  key ^= key >> 33; key *= 0xc4ceb9fe1a85ec53ull;
  key ^= key >> 33;
  return (unsigned)key & t.mask;
}

// the slot of `key`, claimed when the table does not hold it; -1 after capacity probes (the caller raises the error word)
__device__ __forceinline__ int find_or_claim(const Table& t, u64 key, u64* __restrict__ stat)
{
  const u64 want = key | kOccupied;
  unsigned s = home_slot(t, key);
  for (unsigned probe = 0; probe <= t.mask; ++probe, s = (s + 1u) & t.mask)
  {
    u64* kp = &t.slots[s].key;
    u64 cur = __hip_atomic_load(kp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == 0ull)
    {
      cur = atomicCAS(kp, 0ull, want);
      if (cur == 0ull)
      {
        atomicAdd(&stat[kStatOccupied], 1ull);
        return (int)s;
      }
    }
    if (cur == want) return (int)s;
  }
  return -1;
}

// the slot of `key`, -1 when the table does not hold it: read-only, until the key or an empty slot, capacity probes at most
__device__ __forceinline__ int find(const Table& t, u64 key)
{
  const u64 want = key | kOccupied;
  unsigned s = home_slot(t, key);
  for (unsigned probe = 0; probe <= t.mask; ++probe, s = (s + 1u) & t.mask)
  {
    const u64 cur = __hip_atomic_load(&t.slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == want) return (int)s;
    if (cur == 0ull) return -1;
  }
  return -1;
}

// what the exports hand out and a prune keeps: frames >= min_frames and, for a ratio >= 0, misses <= ratio * frames
struct Keep
{
  const unsigned* miss;  // null: no voxel has a miss
  unsigned min_frames;
  double ratio;
  __device__ bool operator()(const Slot& S, unsigned i) const
  {
    if (S.key == 0ull || S.frames < min_frames) return false;
    if (!(ratio >= 0.)) return true;
    return (double)(miss ? miss[i] : 0u) <= ratio * (double)S.frames;
  }
};

struct FrameMove
{
  int fused;        // 0: the points are world points already
  int interpolate;
  InterpConst c;
  Rigid R;
  double time_offset;
};

// ---- the walk of a ray through the voxels (DenseMapHost.carve and .cast, dense_ray_steps: statement for statement, in double,
// without contraction -- the units are built with -ffp-contract=off)
struct Ray
{
  long long i[3], left[3], step[3];  // the voxel, the steps left and their direction per axis
  double tmax[3], tdelta[3];         // the parameter in [0, 1] at which the ray leaves the voxel along each axis, and its step
  long long total;                   // steps of the whole walk
  double len, tt;                    // |p - o|, and how far along it the walk goes, in metres
};

// the ray from o towards p that ends at min(len + reach_add, range) (the carve: reach_add = -margin; a cast: +extend); false
// when it casts none: a coordinate not finite, tt not > 0, len 0, a start or end index outside [-2^20, 2^20)
__device__ __forceinline__ bool dense_ray_begin(const double o[3], const double p[3], double reach_add, double range, double leaf, long long max_steps, Ray& r)
{
  const double d[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
  r.len = __builtin_sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  const double reach = r.len + reach_add;
  r.tt = reach < range ? reach : range;
  bool ok = __builtin_isfinite(o[0]) && __builtin_isfinite(o[1]) && __builtin_isfinite(o[2]) && __builtin_isfinite(p[0]) && __builtin_isfinite(p[1]) &&
            __builtin_isfinite(p[2]) && r.tt > 0. && r.len > 0.;
  const double scale = r.tt / r.len;
  double e[3], f0[3], f1[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    e[k] = o[k] + d[k] * scale;
    f0[k] = __builtin_floor(o[k] / leaf);
    f1[k] = __builtin_floor(e[k] / leaf);
    ok = ok && f0[k] >= -kIndexRange && f0[k] < kIndexRange && f1[k] >= -kIndexRange && f1[k] < kIndexRange;
  }
  r.total = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k)
  {
    r.i[k] = ok ? (long long)f0[k] : 0ll;
    const long long i1 = ok ? (long long)f1[k] : 0ll;
    r.left[k] = i1 > r.i[k] ? i1 - r.i[k] : r.i[k] - i1;
    r.step[k] = i1 > r.i[k] ? 1 : (i1 < r.i[k] ? -1 : 0);
    r.tmax[k] = 0.;
    r.tdelta[k] = 0.;
    if (r.left[k] > 0)
    {
      const double span = e[k] - o[k];
      r.tmax[k] = ((double)(r.i[k] + (r.step[k] > 0 ? 1 : 0)) * leaf - o[k]) / span;
      r.tdelta[k] = leaf / __builtin_fabs(span);
    }
    r.total += r.left[k];
  }
  if (r.total > max_steps) r.total = max_steps;  // (never: the ray is no longer than the range)
  return ok;
}

__device__ __forceinline__ u64 dense_ray_key(const Ray& r)
{
  return ((u64)(r.i[2] + 1048576ll) << 42) | ((u64)(r.i[1] + 1048576ll) << 21) | (u64)(r.i[0] + 1048576ll);
}

// the axis of the next step: the smallest tmax among those with steps left, ties to x, then y; -1 when none is left.
// best: that tmax -- the parameter at which the ray leaves the voxel it is in
__device__ __forceinline__ int dense_ray_next(const Ray& r, double& best)
{
  int ax = -1;
  best = 0.;
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (r.left[q] > 0 && (ax < 0 || r.tmax[q] < best)) { ax = q; best = r.tmax[q]; }
  return ax;
}

// one step along ax (indexed by a run-time axis, written out: no private array leaves the registers)
__device__ __forceinline__ void dense_ray_step(Ray& r, int ax)
{
  if (ax == 0) { r.i[0] += r.step[0]; r.tmax[0] += r.tdelta[0]; r.left[0] -= 1; }
  else if (ax == 1) { r.i[1] += r.step[1]; r.tmax[1] += r.tdelta[1]; r.left[1] -= 1; }
  else { r.i[2] += r.step[2]; r.tmax[2] += r.tdelta[2]; r.left[2] -= 1; }
}
}  // namespace dense
}  // namespace lsa

struct lsa_dense_map
{
  using Slot = lsa::dense::Slot;
  using u64 = lsa::u64;
  lsa_ctx* ctx = nullptr;
  hipStream_t stream = nullptr;  // the context's look-ahead stream
  double leaf = 0.1;
  Slot* slots = nullptr;
  int* source = nullptr;  // [capacity], beside the slots
  unsigned* miss = nullptr;  // [2 * capacity] misses and miss-frame words, from the first carve on
  unsigned capacity = 0;
  unsigned initial_capacity = 1u << 16;
  size_t max_bytes = lsa::dense::kDefaultMaxBytes;
  int stress = 0;
  u64* stat = nullptr;        // device, kStatWords
  u64* host_words = nullptr;  // coherent host memory, 4 words
  int* slot_of = nullptr;     // [slot_cap] the slot of every point of the call in flight
  int slot_cap = 0;
  lsa_point_t* staged = nullptr;  // lsa_dense_map_insert_points: the caller's points on the device
  int staged_cap = 0;
  hipEvent_t ev_frame = nullptr;  // the context's stream up to the frame the fused insertion reads
  // the host's bound of the occupied slots: the last count the device published plus the points inserted since
  unsigned next_serial = 1, epoch = 1, seen_serial = 0;
  unsigned known = 0;
  std::deque<std::pair<unsigned, int>> pending;
  long long pending_sum = 0;
  int last_frame = INT32_MIN;
  int rehashes = 0;
  // export scratch, kept between exports
  int* chunks = nullptr; int chunks_cap = 0;
  int* totals = nullptr;  // device, 2 ints: the total and the compaction's aside slot
  u64* keys[2] = {nullptr, nullptr}; unsigned* index[2] = {nullptr, nullptr}; int keys_cap = 0;
  void* sort_tmp = nullptr; size_t sort_tmp_cap = 0;
  lsa_point_t* out_pts = nullptr; lsa_dense_voxel_t* out_vox = nullptr; int* out_src = nullptr; unsigned* out_miss = nullptr; int out_cap = 0;
  double export_seconds = 0.;
  // re-projections (lsa_dense_map_reproject)
  int reprojections = 0;
  long long dropped = 0;  // voxels, since the last clear
  double reproject_seconds = 0.;
  // free space (lsa_dense_map_carve_*, lsa_dense_map_prune)
  double carve_margin_leaves = 2., carve_range = 30.;
  int carve_stride = 1;
  float* staged_origins = nullptr;  // lsa_dense_map_carve_points: the caller's origins on the device
  int staged_origins_cap = 0;
  double carve_seconds = 0.;  // the host's, of the last carve call: what enqueueing it cost
  long long pruned = 0;       // voxels, since the last clear
  int prunes = 0;
  // normals (lsa_dense_map_get_normals): the call's viewpoints and records on the device
  float* viewpoints = nullptr; int viewpoints_cap = 0;
  unsigned* out_normals = nullptr; int out_normals_cap = 0;  // 5 words a record
  double* normal_sums = nullptr; int normal_sums_cap = 0;    // 9 a voxel, between the two launches
  double normals_seconds = 0.;
  // the floor plan (lsa_dense_map_get_grid): the rasters, records and states of the last call, kept for the next
  long long grid_max_cells = 1ll << 24;
  unsigned char* grid_scratch = nullptr; size_t grid_scratch_cap = 0;
  int* grid_box = nullptr;  // device, 4 ints
  double grid_seconds = 0.;
  // rays (lsa_dense_cast.hip): the inputs and outputs of the last call on the device, kept for the next
  unsigned char* cast_scratch = nullptr; size_t cast_scratch_cap = 0;
  double cast_seconds = 0.;  // the host's, of the last call
};

namespace lsa
{
namespace dense
{
inline Table table_of(const lsa_dense_map* dm) { return Table{dm->slots, dm->source, dm->miss, dm->capacity - 1u, dm->stress}; }
int settle(lsa_dense_map* dm, const char* who);  // lsa_dense_map.hip: waits for the insertions and carves in flight
double now_seconds();                            // lsa_dense_map.hip
}  // namespace dense
}  // namespace lsa
