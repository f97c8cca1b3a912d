// lsa_dense_table.h -- what the units of the dense map share (lsa_dense_*.hip).  Device side: the slot and its key, the table
// and its look-ups, the export's predicate, the counts and how they are published, the move of a frame point to the world, and
// the walk of a ray through the voxels.  Host side, the lower half: the map's host object and the host functions more than one
// unit calls, each under the unit that defines it.  Internal: HIP units only.
//
// The table is an open-addressing hash table in HBM, capacity a power of two, one 64-byte slot per voxel:
//   key   u64   0 = empty, otherwise bit 63 | ((iz + 2^20) << 42) | ((iy + 2^20) << 21) | (ix + 2^20); claimed with a 64-bit CAS
//   cand  u64   the call's candidate word (ordered intensity << 32) | ~index, 0 between two calls
//   point 32 B  the voxel's LidarPoint
//   count, frames, first_frame, last_frame
// Beside the slots, source[capacity]: the ordinal of the call whose point the voxel holds (the 64-byte slot is full), and,
// from the first carve on, miss[2 * capacity]: the voxel's misses, then the word of the last ordinal that counted one.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <deque>
#include <initializer_list>
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

constexpr unsigned kQuietNaN = 0x7fc00000u;  // the word of "no value" in a record of floats (a normal, a cell)

// the order-preserving code of an intensity: f2ou, and 0 -- below -inf -- for a NaN
__device__ __forceinline__ unsigned intensity_code(float v) { return v == v ? f2ou(v) : 0u; }

// ---- the key (without bit 63): 3 x 21 bits, every index of [-2^20, 2^20) moved up by 2^20; z first, as the key holds them.
// T: long long, or the double that holds a whole number in range.  A template on purpose: voxel_key's doubles must be converted
// here, one axis after the other -- converting them at the call reorders instructions of k_dense_claim and k_dense_move, whose
// streams scripts/compare_device_code.py holds to what they were
constexpr long long kIndexBias = 1048576ll;
template <typename T>
__device__ __forceinline__ u64 pack_key(T iz, T iy, T ix)
{
  return ((u64)((long long)iz + kIndexBias) << 42) | ((u64)((long long)iy + kIndexBias) << 21) | (u64)((long long)ix + kIndexBias);
}
// the index along axis 0, 1, 2 = x, y, z
__device__ __forceinline__ long long key_index(u64 key, int axis) { return (long long)((key >> (21 * axis)) & 0x1fffffull) - kIndexBias; }

// the key of a cell given by its indices; false outside the range
__device__ __forceinline__ bool cell_key(long long ix, long long iy, long long iz, u64& key)
{
  if (ix < -kIndexBias || ix >= kIndexBias || iy < -kIndexBias || iy >= kIndexBias || iz < -kIndexBias || iz >= kIndexBias) return false;
  key = pack_key(iz, iy, ix);
  return true;
}

__device__ __forceinline__ bool voxel_key(const float4& a, double leaf, u64& key)
{
  if (!(__builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z))) return false;
  const double ix = __builtin_floor((double)a.x / leaf), iy = __builtin_floor((double)a.y / leaf), iz = __builtin_floor((double)a.z / leaf);
  if (!(ix >= -kIndexRange && ix < kIndexRange && iy >= -kIndexRange && iy < kIndexRange && iz >= -kIndexRange && iz < kIndexRange)) return false;
  key = pack_key(iz, iy, ix);
  return true;
}

// first_frame / last_frame and the ordinal of a miss are folded with atomicMax on words under which the zeroed word is the
// identity: a larger last_frame has a larger word, a smaller first_frame has a larger word
__device__ __forceinline__ unsigned last_word(int v) { return (unsigned)v ^ 0x80000000u; }
__device__ __forceinline__ unsigned first_word(int v) { return ~((unsigned)v ^ 0x80000000u); }
__device__ __forceinline__ int last_of_word(unsigned w) { return (int)(w ^ 0x80000000u); }
__device__ __forceinline__ int first_of_word(unsigned w) { return (int)(~w ^ 0x80000000u); }

// one add a wavefront for the lanes with `mine`; every lane of the wavefront that has not returned calls it
__device__ __forceinline__ void add_once_a_wavefront(u64* word, bool mine)
{
  const u64 those = __ballot(mine);
  if (mine && (int)(threadIdx.x & 63) == __ffsll((long long)those) - 1) atomicAdd(word, (u64)__popcll(those));
}

// The counts to the coherent host words, by one thread, after the launch before has left them final: [1] error, [2] skipped,
// ([3] the voxels a re-projection dropped,) and last, as the release the host's acquire pairs with, [0] = serial << 32 | occupied
__device__ __forceinline__ void publish_counts(const u64* stat, u64* host_words, unsigned serial, bool dropped)
{
  __hip_atomic_store(&host_words[1], stat[kStatError], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host_words[2], stat[kStatSkipped], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (dropped) __hip_atomic_store(&host_words[3], stat[kStatDropped], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host_words[0], ((u64)serial << 32) | (stat[kStatOccupied] & 0xffffffffull), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
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

__device__ __forceinline__ u64 dense_ray_key(const Ray& r) { return pack_key(r.i[2], r.i[1], r.i[0]); }

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
  // export scratch, kept between exports (the caps of what `room` grows: elements, or bytes of a buffer of bytes)
  int* chunks = nullptr; int chunks_cap = 0;
  int* totals = nullptr;  // device, 2 ints: the total and the compaction's aside slot
  u64* keys[2] = {nullptr, nullptr}; unsigned* index[2] = {nullptr, nullptr}; size_t keys_cap = 0;
  unsigned char* sort_tmp = nullptr; size_t sort_tmp_cap = 0;
  lsa_point_t* out_pts = nullptr; lsa_dense_voxel_t* out_vox = nullptr; int* out_src = nullptr; unsigned* out_miss = nullptr; size_t out_cap = 0;
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

// ---- lsa_dense_map.hip: the table's life
double now_seconds();
// waits for the insertions and carves in flight; a probe sequence that ran out is reported here
int settle(lsa_dense_map* dm, const char* who);
// LSA_E_STATE when a probe sequence has run through the whole table (the device's error word, as last published)
int probe_ran_out(lsa_dense_map* dm, const char* who);
// the host's upper bound of the occupied slots, never waited for; exact after settle
long long occupied_bound(lsa_dense_map* dm);
// everything enqueued up to `serial` has been published and waited for: the bound is the count the device left
inline void adopt_published(lsa_dense_map* dm, unsigned serial)
{
  dm->seen_serial = serial;
  dm->known = (unsigned)__atomic_load_n(&dm->host_words[0], __ATOMIC_ACQUIRE);
  dm->pending.clear();
  dm->pending_sum = 0;
}
// the table with room for n more points: (bound of occupied slots) + n <= capacity / 2, by rehashing into a larger one
int make_room(lsa_dense_map* dm, long long n, const char* who);
// `bytes` of device memory, zeroed behind what the stream holds; null with *e set when the allocation (hipErrorOutOfMemory)
// or the memset is refused -- nothing is left allocated then
void* fresh_zeroed(lsa_dense_map* dm, size_t bytes, hipError_t* e);
// The arrays of a table that is not the map's: a fresh one before the swap, the old one after it.  miss: null in a map never
// carved -- a fresh table comes without, and the swap leaves none to retire
struct TableArrays
{
  Slot* slots;
  int* source;
  unsigned* miss;
  unsigned capacity;
};
// a zeroed table of cap slots with its source array -- and, in a map that has been carved, its miss array --;
// LSA_E_CAPACITY without memory
int fresh_table(lsa_dense_map* dm, unsigned cap, TableArrays* fresh, const char* who, const char* consequence);
// the fresh table becomes the map's; the old one is the caller's to read from and then to retire_dev, array by array
TableArrays swap_table(lsa_dense_map* dm, const TableArrays& fresh);
// One buffer of a group that grows together under one cap: where the map keeps its pointer, and the bytes of an element
struct Buffer
{
  void** at;
  size_t elem;
};
// Room for `count` elements in every device buffer of `group`, whose contents need not survive; what is outgrown goes to the
// graveyard.  The new cap is count + count / slack (slack 0: count).  LSA_E_CAPACITY without memory (the cap is then 0, and the
// next call retires what the group did get), `advice` behind the figure
int room(lsa_dense_map* dm, std::initializer_list<Buffer> group, size_t* cap, size_t count, size_t slack, const char* who, const char* what, const char* advice = "");
// the move of the context's frame to the world inside a fused kernel
FrameMove frame_move(int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset);
// A fused launch reads the context's frame as the context's stream has left it so far (hold_frame, before the launch), and
// the buffer is then held until the launch is over by an event its next writer waits for (frame_writer_guard), never by the
// host: release_frame, behind the launch that reads the buffer last
int hold_frame(lsa_dense_map* dm);
int release_frame(lsa_dense_map* dm);
// no ray has more steps, whatever it is given
inline long long ray_max_steps(double range, double leaf) { return 3ll * ((long long)std::ceil(range / leaf) + 2ll); }
// what the exports hand out and a prune keeps
inline Keep keep_of(const lsa_dense_map* dm, int min_frames, double max_miss_ratio) { return Keep{dm->miss, (unsigned)std::max(min_frames, 0), max_miss_ratio}; }

// ---- lsa_dense_export.hip
// keys and slot indices of the voxels that pass, in slot order, left in dm->keys[0] / index[0]; returns their number.  The
// map must be settled.
int compact_kept(lsa_dense_map* dm, int min_frames, double max_miss_ratio, const char* who);
// the voxels that pass (Keep) in ascending key order, left in dm->out_pts / out_vox / out_src / out_miss (and their keys and
// slots in dm->keys[1] / index[1]); returns their number
int export_sorted(lsa_dense_map* dm, int min_frames, double max_miss_ratio, const char* who);
}  // namespace dense
}  // namespace lsa
