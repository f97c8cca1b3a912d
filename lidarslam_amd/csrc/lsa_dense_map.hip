// lsa_dense_map.hip -- the dense point-cloud map: registered frames voxel-hashed on the device (the host
// statement the table is held to, byte for byte, is DenseMapHost in lidarslam_amd/_dense_map.py).
//
// An open-addressing hash table in HBM, capacity a power of two, one 64-byte slot per voxel:
//   key   u64   0 = empty, otherwise bit 63 | ((iz + 2^20) << 42) | ((iy + 2^20) << 21) | (ix + 2^20); claimed with a 64-bit CAS
//   cand  u64   the call's candidate word (ordered intensity << 32) | ~index, 0 between two calls
//   point 32 B  the voxel's LidarPoint
//   count, frames, first_frame, last_frame
// An insertion's cost is the frame's size, not the map's.  Two launches, one thread per point:
//   k_dense_claim  finds or claims the point's slot, adds 1 to its count, atomicMax'es the candidate word, notes the slot
//   k_dense_apply  the thread whose index the candidate word names applies the new / existing voxel rule and disarms the word
// The kernel boundary is the only synchronisation: no workgroup waits for another, no flag is spun on, and a probe sequence
// is bounded by the capacity (a thread that exhausts it raises the map's error word and returns).  Every rule is
// independent of the order in which the points of a call arrive, which is what lets atomics give the host's bytes.
// The fused form (lsa_dense_map_insert_frame) moves the context's frame to the world inside both kernels with
// frame_point_to_world, k_transform_out's own arithmetic: a world point only reaches memory when it wins its voxel.
// Growth: the host keeps (upper bound of occupied slots) + n <= capacity / 2 from the last count the device left in
// coherent host memory plus the points inserted since -- never waited for --, and k_dense_rehash moves the slots into a
// table of twice the size on the same stream; the old table goes to the context's graveyard.
// Export (not on the frame path): lsa_compact.h's stable compaction of the slots that pass min_frames, rocprim's radix sort
// by key, a gather.
// Beside the slots, source[capacity]: the ordinal of the call whose point the voxel holds (the 64-byte slot is full).  It is
// what lets a corrected trajectory move the map (lsa_dense_map_reproject, not on the frame path either): every voxel's point
// under the correction of the frame that measured it, re-keyed into a fresh table of the same capacity, voxels that meet
// merged -- three launches, one thread per old slot, under the same rules as the insertion:
//   k_dense_move    moves the point, finds or claims its slot in the new table, adds count and frames, folds first / last
//                   and the candidate word (intensity code << 32) | ~ordered(source) in with atomics, notes the new slot
//   k_dense_elect   the old slots whose word the candidate names atomicMin their old key: ties on intensity and source
//   k_dense_settle  the old slot named by both writes the moved point and its source, caps frames, disarms the word
// Free space (DenseMapHost.carve): miss[2 * capacity], made by the first carve -- a map never carved has none and pays for
// none --: the voxel's misses, then the word of the last ordinal that counted one (ordinal ^ 2^31: the zeroed word is "none").
//   k_dense_carve   one thread per ray walks the voxels from the sensor to shortly before the point -- a number of steps
//                   known before the first -- and looks each up without ever claiming; a voxel found whose last_frame is
//                   not the ordinal takes atomicMax on its word, and the one thread that raised it adds the miss
// It runs behind k_dense_apply of its ordinal on the same stream, so last_frame is final.  The array is carried by the rehash,
// merged by the re-projection (atomicAdd, atomicMax), read by the export's predicate; lsa_dense_map_prune is the rehash under
// that predicate into the smallest table that holds what passes.
// Normals (DenseMapHost.normals; not on the frame path, nothing stored): behind the export's compaction and sort
//   k_dense_normals         a group of 32 lanes a voxel probes the surrounding cells, packs the neighbours found into LDS in cell
//                           order and adds the nine sums up in that order
//   k_dense_normal_records  one thread a voxel: covariance, eigen33<double>, the sign towards the viewpoint, the record
// The floor plan (DenseMapHost.grid; not on the frame path, nothing stored, read-only on the table): rasters of one call
//   k_dense_grid_bounds    (no window) the box of the kept voxels' cells
//   k_dense_grid_columns   every kept voxel: atomicMin of its z code into its cell of the extent widened by the radius
//   k_dense_grid_rows / _ground   one thread a cell: the smallest code of the neighbourhood, along the row, then along the column
//   k_dense_grid_band      every kept voxel against the ground of its cell: atomicAdd on a count, atomicMax on the top code
//   k_dense_grid_classify  one thread a cell: the 20-byte record and the state
// The slot, the table, its look-ups, the export's predicate and the walk of a ray are in lsa_dense_table.h, shared with
// lsa_dense_cast.hip (rays that stop at the first voxel that counts: DenseMapHost.cast / .compare).
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <deque>
#include <new>
#include <vector>
#include "lsa_compact.h"
#include "lsa_ctx.h"
#include "lsa_dense_table.h"
#include "lsa_device_grid_io.h"
#include "lsa_device_math.h"
#include "lsa_wave.h"
#include "host/lsa_occupancy.h"
#include "host/lsa_pcd.h"

namespace lsa
{
InterpConst make_interp_const(const double H0[16], const double H1[16], double t0, double t1);  // lsa_transform.hip
}
using namespace lsa;
using namespace lsa::dense;  // the slot, the table and its look-ups, the walk of a ray, the map's host object (lsa_dense_table.h)

namespace
{
// launch 1: slot, count, candidate
__global__ __launch_bounds__(256) void k_dense_claim(const float4* __restrict__ in, int n, const FrameMove m, double leaf, Table t, u64* __restrict__ stat,
                                                     int* __restrict__ slot_of)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 a = in[2 * (size_t)i];
  float4 b = in[2 * (size_t)i + 1];
  if (m.fused) frame_point_to_world(a, b, m.interpolate, m.c, m.R, m.time_offset);
  u64 key = 0;
  const bool ok = voxel_key(a, leaf, key);
  const u64 skipping = __ballot(!ok);
  if (!ok)
  {
    // one add a wavefront
    if ((int)(threadIdx.x & 63) == __ffsll((long long)skipping) - 1) atomicAdd(&stat[kStatSkipped], (u64)__popcll(skipping));
    slot_of[i] = -1;
    return;
  }
  const int s = find_or_claim(t, key, stat);
  slot_of[i] = s;
  if (s < 0)
  {
    atomicOr(&stat[kStatError], 1ull);
    return;
  }
  atomicAdd(&t.slots[s].count, 1u);
  atomicMax(&t.slots[s].cand, ((u64)intensity_code(b.z) << 32) | (u64)(~(unsigned)i));
}

// launch 2: the winner of every voxel of the call applies the rule.  host_words: coherent host memory, [0] = serial << 32 |
// occupied slots, written last, [1] error, [2] skipped -- by one thread, after launch 1 has left them final.
__global__ __launch_bounds__(256) void k_dense_apply(const float4* __restrict__ in, int n, const FrameMove m, Table t, const int* __restrict__ slot_of, int frame,
                                                     const u64* __restrict__ stat, u64* __restrict__ host_words, unsigned serial)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0)
  {
    __hip_atomic_store(&host_words[1], stat[kStatError], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host_words[2], stat[kStatSkipped], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host_words[0], ((u64)serial << 32) | (stat[kStatOccupied] & 0xffffffffull), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (i >= n) return;
  const int s = slot_of[i];
  if (s < 0) return;
  Slot& S = t.slots[s];
  // (only this voxel's winner writes the word during this launch, and the 0 it writes names nobody: an index is never 2^32 - 1)
  const u64 w = __hip_atomic_load(&S.cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if ((unsigned)w != ~(unsigned)i) return;
  float4 a = in[2 * (size_t)i];
  float4 b = in[2 * (size_t)i + 1];
  if (m.fused) frame_point_to_world(a, b, m.interpolate, m.c, m.R, m.time_offset);
  if (S.frames == 0u)
  {
    S.a = a; S.b = b;
    t.source[s] = frame;
    S.frames = 1u;
    S.first = S.last = frame;
  }
  else
  {
    if (S.last != frame) { S.frames += 1u; S.last = frame; }
    if ((unsigned)(w >> 32) > intensity_code(S.b.z)) { S.a = a; S.b = b; t.source[s] = frame; }  // strictly greater: the earlier frame keeps a tie
  }
  S.cand = 0ull;
}

// every occupied slot of the old table into the new one (zeroed); keys are unique, so a slot is only ever claimed from empty
// (a prune is this launch under its `keep`; growth's keeps every voxel.  old_miss: null in a map never carved)
__global__ __launch_bounds__(256) void k_dense_rehash(const Slot* __restrict__ old, const int* __restrict__ old_source, const unsigned* __restrict__ old_miss,
                                                      unsigned old_capacity, Keep keep, Table t, u64* __restrict__ stat)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_capacity) return;
  const Slot o = old[i];
  if (o.key == 0ull) return;
  if (!keep(o, i)) return;
  unsigned s = home_slot(t, o.key & ~kOccupied);
  for (unsigned probe = 0; probe <= t.mask; ++probe, s = (s + 1u) & t.mask)
  {
    if (atomicCAS(&t.slots[s].key, 0ull, o.key) != 0ull) continue;
    Slot& S = t.slots[s];
    S.a = o.a; S.b = o.b;
    S.count = o.count; S.frames = o.frames; S.first = o.first; S.last = o.last;
    t.source[s] = old_source[i];
    if (old_miss)
    {
      t.miss[s] = old_miss[i];
      t.miss[(size_t)t.mask + 1u + s] = old_miss[(size_t)old_capacity + i];
    }
    return;
  }
  atomicOr(&stat[kStatError], 1ull);
}

// the occupied count of a table whose slots the host counted (a prune), published as k_dense_apply publishes
__global__ void k_dense_publish(u64* __restrict__ stat, u64* __restrict__ host_words, unsigned serial, unsigned occupied)
{
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  stat[kStatOccupied] = occupied;
  __hip_atomic_store(&host_words[1], stat[kStatError], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host_words[2], stat[kStatSkipped], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&host_words[0], ((u64)serial << 32) | (u64)occupied, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- free space ------------------------------------------------------------------------------------------------------------
struct Carve
{
  const float* origins;  // unfused: [n_origins][3] world positions of the sensor
  int n_origins;         // 1 or the number of points
  int stride;            // ray r belongs to point r * stride
  int rays;
  int frame;
  double leaf, margin, range;  // margin = margin_leaves * leaf
  long long max_steps;         // 3 * (ceil(range / leaf) + 2): no ray has more, whatever it is given
};

// DenseMapHost.carve, statement for statement: double, no contraction (the unit is built with -ffp-contract=off)
__global__ __launch_bounds__(256) void k_dense_carve(const float4* __restrict__ in, const FrameMove m, const Carve c, Table t, u64* __restrict__ stat)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= c.rays) return;
  const size_t at = (size_t)r * (size_t)c.stride;
  float4 a = in[2 * at];
  float4 b = in[2 * at + 1];
  float ofx, ofy, ofz;
  if (m.fused)
  {
    // the sensor at the time the point was measured: what the frame's own origin becomes under the point's pose
    float4 oa = make_float4(0.f, 0.f, 0.f, a.w), ob = b;
    frame_point_to_world(oa, ob, m.interpolate, m.c, m.R, m.time_offset);
    frame_point_to_world(a, b, m.interpolate, m.c, m.R, m.time_offset);
    ofx = oa.x; ofy = oa.y; ofz = oa.z;
  }
  else
  {
    const float* o = c.origins + (c.n_origins == 1 ? (size_t)0 : 3 * at);
    ofx = o[0]; ofy = o[1]; ofz = o[2];
  }
  const double o[3] = {(double)ofx, (double)ofy, (double)ofz};
  const double p[3] = {(double)a.x, (double)a.y, (double)a.z};
  // the set-up and the step of the walk: dense_ray_begin / _next / _step of lsa_dense_table.h, shared with the casts
  Ray ray;
  const bool ok = dense_ray_begin(o, p, -c.margin, c.range, c.leaf, c.max_steps, ray);
  const u64 casting = __ballot(ok);
  if (!ok) return;
  // one add a wavefront
  if ((int)(threadIdx.x & 63) == __ffsll((long long)casting) - 1) atomicAdd(&stat[kStatRays], (u64)__popcll(casting));
  const unsigned word = (unsigned)c.frame ^ 0x80000000u;
  unsigned* __restrict__ words = t.miss + (size_t)t.mask + 1u;
  for (long long k = 0;; ++k)
  {
    const int s = find(t, dense_ray_key(ray));
    // (last_frame is final: k_dense_apply of this ordinal ran before this launch)
    if (s >= 0 && t.slots[s].last != c.frame && atomicMax(&words[s], word) < word) atomicAdd(&t.miss[s], 1u);
    if (k >= ray.total) break;
    double best;
    const int ax = dense_ray_next(ray, best);
    if (ax < 0) break;  // (never: total is the sum of what is left)
    dense_ray_step(ray, ax);
  }
}

// ---- re-projection under a corrected trajectory --------------------------------------------------------------------------
// The scratch of one re-projection, [capacity] each: pick (armed ~0: the smallest old key among the winners of a new voxel),
// frames (the sum of the merged voxels' frames, in 64 bits), to (the new slot of every old one; -1: empty, dropped, no slot).
struct Reproject
{
  const Slot* old;
  const int* old_source;
  const unsigned* old_miss;  // null in a map never carved
  unsigned old_capacity;
  const double* corrections;  // [n][16] row-major; entry j belongs to ordinal first_frame + j
  int first_frame, n;
  double leaf;
  u64* pick;
  u64* frames;
  int* to;
};

// first_frame / last_frame of a slot of the new table are folded with atomicMax on words under which the zeroed slot is the
// identity: a larger last_frame has a larger word, a smaller first_frame has a larger word.  k_dense_settle decodes them.
__device__ __forceinline__ unsigned last_word(int v) { return (unsigned)v ^ 0x80000000u; }
__device__ __forceinline__ unsigned first_word(int v) { return ~((unsigned)v ^ 0x80000000u); }
// largest intensity code, then the smaller source (signed)
__device__ __forceinline__ u64 merge_word(const float4& b, int source) { return ((u64)intensity_code(b.z) << 32) | (u64)first_word(source); }

// rigid_apply under the correction of the frame that measured the point, narrowed to float; w is kept
__device__ __forceinline__ float4 reprojected(const Reproject& r, const float4& a, int source)
{
  long long c = (long long)source - (long long)r.first_frame;
  c = c < 0 ? 0 : (c > (long long)r.n - 1 ? (long long)r.n - 1 : c);
  const double* T = r.corrections + 16 * c;
  Rigid g;
  for (int row = 0; row < 3; ++row)
  {
    for (int col = 0; col < 3; ++col) g.R[3 * row + col] = T[4 * row + col];
    g.t[row] = T[4 * row + 3];
  }
  double ox, oy, oz;
  rigid_apply(g, (double)a.x, (double)a.y, (double)a.z, ox, oy, oz);
  return make_float4((float)ox, (float)oy, (float)oz, a.w);
}

// launch 1: every occupied old slot moves its point, finds or claims the voxel it falls into, and folds its record in
__global__ __launch_bounds__(256) void k_dense_move(const Reproject r, Table t, u64* __restrict__ stat)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.old_capacity) return;
  const Slot& o = r.old[i];
  if (o.key == 0ull) { r.to[i] = -1; return; }
  const int source = r.old_source[i];
  const float4 a = reprojected(r, o.a, source);
  u64 key = 0;
  if (!voxel_key(a, r.leaf, key))
  {
    atomicAdd(&stat[kStatDropped], 1ull);
    r.to[i] = -1;
    return;
  }
  const int s = find_or_claim(t, key, stat);
  r.to[i] = s;
  if (s < 0)
  {
    atomicOr(&stat[kStatError], 1ull);
    return;
  }
  Slot& S = t.slots[s];
  atomicAdd(&S.count, o.count);
  atomicAdd(&r.frames[s], (u64)o.frames);
  atomicMax(reinterpret_cast<unsigned*>(&S.first), first_word(o.first));
  atomicMax(reinterpret_cast<unsigned*>(&S.last), last_word(o.last));
  atomicMax(&S.cand, merge_word(o.b, source));
  if (r.old_miss)
  {
    // misses add up modulo 2^32; the larger ordinal has the larger word and the zeroed word, "none", is the identity
    const unsigned misses = r.old_miss[i], word = r.old_miss[(size_t)r.old_capacity + i];
    if (misses) atomicAdd(&t.miss[s], misses);
    if (word) atomicMax(&t.miss[(size_t)t.mask + 1u + s], word);
  }
}

// launch 2: among the old voxels the candidate word names -- equal intensity code and source -- the smallest old key
__global__ __launch_bounds__(256) void k_dense_elect(const Reproject r, Table t)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= r.old_capacity) return;
  const int s = r.to[i];
  if (s < 0) return;
  const Slot& o = r.old[i];
  const u64 w = __hip_atomic_load(&t.slots[s].cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (w == merge_word(o.b, r.old_source[i])) atomicMin(&r.pick[s], o.key);
}

// launch 3: the old voxel named by both gives the new one its point and source and finishes its record; one thread
// publishes the counts as k_dense_apply does ([3]: the voxels dropped)
__global__ __launch_bounds__(256) void k_dense_settle(const Reproject r, Table t, const u64* __restrict__ stat, u64* __restrict__ host_words, unsigned serial)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0)
  {
    __hip_atomic_store(&host_words[1], stat[kStatError], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host_words[2], stat[kStatSkipped], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host_words[3], stat[kStatDropped], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host_words[0], ((u64)serial << 32) | (stat[kStatOccupied] & 0xffffffffull), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (i >= r.old_capacity) return;
  const int s = r.to[i];
  if (s < 0) return;
  const Slot& o = r.old[i];
  const int source = r.old_source[i];
  Slot& S = t.slots[s];
  // (only this voxel's winner writes its slot during this launch.  A loser may read the 0 the winner leaves in the word and
  //  find it equal to its own; the pick, which nobody writes here, holds a key that is not the loser's: old keys are unique)
  const u64 w = __hip_atomic_load(&S.cand, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (w != merge_word(o.b, source) || r.pick[s] != o.key) return;
  S.a = reprojected(r, o.a, source);
  S.b = o.b;
  t.source[s] = source;
  const unsigned fw = __builtin_bit_cast(unsigned, S.first), lw = __builtin_bit_cast(unsigned, S.last);
  const int first = (int)(~fw ^ 0x80000000u), last = (int)(lw ^ 0x80000000u);
  S.first = first;
  S.last = last;
  const u64 span = (u64)((long long)last - (long long)first + 1ll), sum = r.frames[s];
  S.frames = (unsigned)(sum < span ? sum : span);
  S.cand = 0ull;
}

// ---- export -------------------------------------------------------------------------------------------------------------
struct ExportPred
{
  const Slot* slots;
  Keep keep;
  __device__ bool operator()(int i) const { return keep(slots[i], (unsigned)i); }
};
struct ExportEmit
{
  const Slot* slots;
  u64* keys;
  unsigned* index;
  __device__ void operator()(int i, int pos) const
  {
    keys[pos] = slots[i].key & ~kOccupied;
    index[pos] = (unsigned)i;
  }
};
__global__ __launch_bounds__(256) void k_dense_gather(const Slot* __restrict__ slots, const int* __restrict__ source, const unsigned* __restrict__ miss,
                                                      const u64* __restrict__ keys, const unsigned* __restrict__ index, int n, float4* __restrict__ pts,
                                                      lsa_dense_voxel_t* __restrict__ voxels, int* __restrict__ sources, unsigned* __restrict__ misses)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Slot& S = slots[index[j]];
  sources[j] = source[index[j]];
  misses[j] = miss ? miss[index[j]] : 0u;
  pts[2 * (size_t)j] = S.a;
  pts[2 * (size_t)j + 1] = S.b;
  lsa_dense_voxel_t v;
  v.key = keys[j];
  v.count = S.count; v.frames = S.frames; v.first_frame = S.first; v.last_frame = S.last;
  voxels[j] = v;
}

// ---- normals (DenseMapHost.normals; not on the frame path) ------------------------------------------------------------------
// One group of 32 lanes a voxel of the sorted export.  The (2r + 1)^3 cells are probed a round of 32 at a time -- independent
// scattered loads, in flight together -- and the points of the neighbours found are packed into LDS in cell order (ballot,
// prefix popcount).  The nine sums must come out in that order, so nine lanes each add one of them up serially over the
// packed list and leave them in memory (72 B a voxel); a second launch, one thread a voxel, runs the covariance,
// eigen33<double>, the flip and the store with every lane at work.  Read-only on the table, no atomics, no loop but find's
// bounded probe and the cells.
struct Normals
{
  const u64* keys;          // [n] ascending: the voxels that pass
  const unsigned* index;    // [n] their slots
  int n;
  int r;                    // radius in leaves: 1 or 2
  unsigned min_neighbors;
  const float* viewpoints;  // [n_viewpoints][3]; null: eigen33's own sign
  int n_viewpoints, first_frame;
  Keep keep;
};
constexpr int kNormalLanes = 32, kNormalGroups = 8, kNormalCells = 125;
constexpr unsigned kNoNormal = 0x7fc00000u;

__device__ __forceinline__ bool cell_key(long long ix, long long iy, long long iz, u64& key)
{
  if (ix < -1048576ll || ix >= 1048576ll || iy < -1048576ll || iy >= 1048576ll || iz < -1048576ll || iz >= 1048576ll) return false;
  key = ((u64)(iz + 1048576ll) << 42) | ((u64)(iy + 1048576ll) << 21) | (u64)(ix + 1048576ll);
  return true;
}

// steps 4 to 7 of the definition: the record of a voxel from its count and sums
__device__ __forceinline__ void normal_record(const Normals& c, const Table& t, unsigned slot, const double p[3], unsigned k, const double s[3], const double S[6],
                                              unsigned* __restrict__ o)
{
  o[4] = k;
  o[0] = o[1] = o[2] = o[3] = kNoNormal;
  if (k < c.min_neighbors) return;
  const double kk = (double)k;
  const double mx = s[0] / kk, my = s[1] / kk, mz = s[2] / kk;
  const Sym3<double> cov = {S[0] / kk - mx * mx, S[1] / kk - mx * my, S[2] / kk - mx * mz, S[3] / kk - my * my, S[4] / kk - my * mz, S[5] / kk - mz * mz};
  Vec3<double> e0, e1, e2;
  double l0, l1, l2;
  eigen33<double>(cov, e0, e1, e2, l0, l1, l2);
  if (!(__builtin_isfinite(l0) && __builtin_isfinite(l1) && __builtin_isfinite(l2) && __builtin_isfinite(e0.x) && __builtin_isfinite(e0.y) && __builtin_isfinite(e0.z))) return;
  if (c.viewpoints && c.n_viewpoints > 0)
  {
    long long at = (long long)t.source[slot] - (long long)c.first_frame;
    at = at < 0 ? 0 : (at > (long long)c.n_viewpoints - 1 ? (long long)c.n_viewpoints - 1 : at);
    const float* v = c.viewpoints + 3 * at;
    const double wx = (double)v[0] - p[0], wy = (double)v[1] - p[1], wz = (double)v[2] - p[2];
    const double dot = (e0.x * wx + e0.y * wy) + e0.z * wz;
    if (dot < 0.) { e0.x = -e0.x; e0.y = -e0.y; e0.z = -e0.z; }
  }
  const double sum = (l0 + l1) + l2;
  const float curvature = sum > 0. ? (float)__builtin_fabs(l0 / sum) : 0.f;
  o[0] = __builtin_bit_cast(unsigned, (float)e0.x);
  o[1] = __builtin_bit_cast(unsigned, (float)e0.y);
  o[2] = __builtin_bit_cast(unsigned, (float)e0.z);
  o[3] = __builtin_bit_cast(unsigned, curvature);
}

__global__ __launch_bounds__(kNormalLanes * kNormalGroups) void k_dense_normals(const Normals c, Table t, double* __restrict__ sums, unsigned* __restrict__ out)
{
  __shared__ float near_q[kNormalGroups][kNormalCells][3];
  const int lane = (int)threadIdx.x & (kNormalLanes - 1), group = (int)threadIdx.x / kNormalLanes;
  const int j = (int)blockIdx.x * kNormalGroups + group;
  const bool live = j < c.n;  // (the same for the lanes of a group; nobody leaves before the barrier)
  long long ix = 0, iy = 0, iz = 0;
  unsigned slot = 0;
  double p[3] = {0., 0., 0.};
  if (live)
  {
    const u64 key = c.keys[j];
    slot = c.index[j];
    ix = (long long)(key & 0x1fffffull) - 1048576ll;
    iy = (long long)((key >> 21) & 0x1fffffull) - 1048576ll;
    iz = (long long)((key >> 42) & 0x1fffffull) - 1048576ll;
    const float4 a = t.slots[slot].a;
    p[0] = (double)a.x; p[1] = (double)a.y; p[2] = (double)a.z;
  }
  const int side = 2 * c.r + 1, cells = side * side * side;
  unsigned k = 0;
  for (int base = 0; base < cells; base += kNormalLanes)
  {
    const int cell = base + lane;
    bool found = false;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    u64 key = 0;
    if (live && cell < cells && cell_key(ix + (cell % side - c.r), iy + ((cell / side) % side - c.r), iz + (cell / (side * side) - c.r), key))
    {
      const int s = find(t, key);
      if (s >= 0 && c.keep(t.slots[s], (unsigned)s))
      {
        found = true;
        q = t.slots[s].a;
      }
    }
    // the group's half of the wavefront's ballot
    const unsigned mine = (unsigned)(__ballot(found) >> (threadIdx.x & 32u));
    if (found)
    {
      const unsigned at = k + (unsigned)__popc(mine & ((1u << lane) - 1u));
      near_q[group][at][0] = q.x; near_q[group][at][1] = q.y; near_q[group][at][2] = q.z;
    }
    k += (unsigned)__popc(mine);
  }
  __syncthreads();
  // lanes 0..2: s_x s_y s_z; lanes 3..8: S_xx S_xy S_xz S_yy S_yz S_zz
  const int a = lane < 3 ? lane : (lane < 6 ? 0 : (lane < 8 ? 1 : 2));
  const int b = lane < 3 ? lane : (lane == 3 ? 0 : (lane == 4 || lane == 6 ? 1 : 2));
  const double pa = a == 0 ? p[0] : (a == 1 ? p[1] : p[2]), pb = b == 0 ? p[0] : (b == 1 ? p[1] : p[2]);
  double acc = 0.;
  if (live && lane < 9)
  {
    if (lane < 3)
      for (unsigned i = 0; i < k; ++i) acc += (double)near_q[group][i][a] - pa;
    else
      for (unsigned i = 0; i < k; ++i)
      {
        const double da = (double)near_q[group][i][a] - pa, db = (double)near_q[group][i][b] - pb;
        acc += da * db;
      }
  }
  // (one lane a voxel for what follows would leave 31 of 32 idle through eigen33: the sums go to memory, and
  //  k_dense_normal_records picks them up with every lane at work)
  if (live && lane < 9) sums[9 * (size_t)j + lane] = acc;
  if (live && lane == 0) out[5 * (size_t)j + 4] = k;
}

// launch 2 of the normals, one thread a voxel: the record from the count and the sums k_dense_normals left
__global__ __launch_bounds__(256) void k_dense_normal_records(const Normals c, Table t, const double* __restrict__ sums, unsigned* __restrict__ out)
{
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= c.n) return;
  const unsigned slot = c.index[j];
  const float4 a = t.slots[slot].a;
  const double p[3] = {(double)a.x, (double)a.y, (double)a.z};
  double v[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) v[i] = sums[9 * (size_t)j + i];
  normal_record(c, t, slot, p, out[5 * (size_t)j + 4], v, v + 3, out + 5 * (size_t)j);
}

// ---- the floor plan (DenseMapHost.grid; not on the frame path, nothing stored) ---------------------------------------------
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
constexpr unsigned kNoCode = ~0u, kAbsent = 0x7fc00000u;

// floor division by a positive b
__device__ __forceinline__ int floor_div(int a, int b)
{
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}
__device__ __forceinline__ void cell_of(u64 key, int cell_leaves, int& cx, int& cy)
{
  cx = floor_div((int)(key & 0x1fffffull) - 1048576, cell_leaves);
  cy = floor_div((int)((key >> 21) & 0x1fffffull) - 1048576, cell_leaves);
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
  o[0] = elevation != kNoCode ? __builtin_bit_cast(unsigned, ou2f(elevation)) : kAbsent;
  o[1] = low != kNoCode ? __builtin_bit_cast(unsigned, ou2f(low)) : kAbsent;
  o[2] = top != 0u ? __builtin_bit_cast(unsigned, ou2f(top)) : kAbsent;
  o[3] = floor_voxels;
  o[4] = obstacle_voxels;
  state[i] = obstacle_voxels >= g.min_obstacle ? (signed char)100 : (floor_voxels >= 1u ? (signed char)0 : (signed char)-1);
}

}  // namespace

namespace
{
long long occupied_bound(lsa_dense_map* dm)
{
  const u64 w = __atomic_load_n(&dm->host_words[0], __ATOMIC_ACQUIRE);
  const unsigned ws = (unsigned)(w >> 32);
  if (ws >= dm->epoch && ws > dm->seen_serial && ws < dm->next_serial)
  {
    dm->seen_serial = ws;
    dm->known = (unsigned)w;
    while (!dm->pending.empty() && dm->pending.front().first <= ws)
    {
      dm->pending_sum -= dm->pending.front().second;
      dm->pending.pop_front();
    }
  }
  return (long long)dm->known + dm->pending_sum;
}

// a zeroed table of cap slots with its source array -- and, in a map that has been carved, its miss array --, zeroed behind
// what the stream holds; LSA_E_CAPACITY without memory
int fresh_table(lsa_dense_map* dm, unsigned cap, Slot** slots, int** source, unsigned** miss, const char* who, const char* consequence)
{
  lsa_ctx* ctx = dm->ctx;
  const size_t bytes = (size_t)cap * sizeof(Slot), source_bytes = (size_t)cap * sizeof(int), miss_bytes = dm->miss ? (size_t)cap * 2 * sizeof(unsigned) : 0;
  *slots = nullptr;
  *source = nullptr;
  *miss = nullptr;
  if (hipMalloc((void**)slots, bytes) != hipSuccess || hipMalloc((void**)source, source_bytes) != hipSuccess ||
      (miss_bytes && hipMalloc((void**)miss, miss_bytes) != hipSuccess))
  {
    (void)hipGetLastError();
    if (*slots) (void)hipFree(*slots);
    if (*source) (void)hipFree(*source);
    *slots = nullptr;
    *source = nullptr;
    *miss = nullptr;
    return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory for a table of " + std::to_string(bytes + source_bytes + miss_bytes) + " bytes; " + consequence);
  }
  hipError_t e = hipMemsetAsync(*slots, 0, bytes, dm->stream);
  if (e == hipSuccess) e = hipMemsetAsync(*source, 0, source_bytes, dm->stream);
  if (e == hipSuccess && miss_bytes) e = hipMemsetAsync(*miss, 0, miss_bytes, dm->stream);
  if (e != hipSuccess)
  {
    (void)hipStreamSynchronize(dm->stream);
    (void)hipFree(*slots);
    (void)hipFree(*source);
    if (*miss) (void)hipFree(*miss);
    *slots = nullptr;
    *source = nullptr;
    *miss = nullptr;
    return ctx->fail(LSA_E_HIP, std::string(who) + ": hipMemsetAsync: " + hipGetErrorString(e));
  }
  return LSA_OK;
}

// the table `fresh` of `cap` slots takes what `keep` lets through of the map's and becomes the map's;
// the old one goes to the graveyard, which launches in flight keep alive (freed by lsa_collect_garbage)
void rehash_into(lsa_dense_map* dm, Slot* fresh, int* fresh_source, unsigned* fresh_miss, unsigned cap, const Keep& keep)
{
  lsa_ctx* ctx = dm->ctx;
  Slot* old = dm->slots;
  int* old_source = dm->source;
  unsigned* old_miss = dm->miss;
  const unsigned old_capacity = dm->capacity;
  dm->slots = fresh;
  dm->source = fresh_source;
  if (fresh_miss) dm->miss = fresh_miss;
  dm->capacity = cap;
  if (!old) return;
  ProfScope ps(ctx, "dense_rehash", (double)old_capacity * (sizeof(Slot) + sizeof(int)) * 2, dm->stream);
  hipLaunchKernelGGL(k_dense_rehash, dim3((old_capacity + 255) / 256), dim3(256), 0, dm->stream, old, old_source, fresh_miss ? old_miss : nullptr, old_capacity, keep,
                     table_of(dm), dm->stat);
  retire_dev(ctx, old);
  retire_dev(ctx, old_source);
  if (fresh_miss) retire_dev(ctx, old_miss);
}

// the table with room for n more points: (bound of occupied slots) + n <= capacity / 2, by rehashing into a larger one
int make_room(lsa_dense_map* dm, long long n, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  const long long need = occupied_bound(dm) + n;
  unsigned cap = dm->capacity ? dm->capacity : dm->initial_capacity;
  // (a first table of "InitialCapacity" slots is a wish, not a demand: under a "MaxBytes" below it the table starts smaller)
  if (!dm->capacity && dm->max_bytes)
    while (cap > kMinCapacity && (size_t)cap * sizeof(Slot) > dm->max_bytes) cap /= 2;
  while ((long long)(cap / 2) < need)
  {
    if (cap >= kMaxCapacity) return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": the table would need more than 2^30 slots");
    cap *= 2;
  }
  if (cap == dm->capacity) return LSA_OK;
  const size_t bytes = (size_t)cap * sizeof(Slot);
  if (dm->max_bytes && bytes > dm->max_bytes)
    return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": a table of " + std::to_string(bytes) + " bytes for " + std::to_string(need) +
                                         " voxels at most is over MaxBytes = " + std::to_string(dm->max_bytes) + "; nothing was inserted");
  Slot* fresh = nullptr;
  int* fresh_source = nullptr;
  unsigned* fresh_miss = nullptr;
  if (const int rc = fresh_table(dm, cap, &fresh, &fresh_source, &fresh_miss, who, "nothing was inserted")) return rc;
  if (dm->slots) dm->rehashes++;
  rehash_into(dm, fresh, fresh_source, fresh_miss, cap, Keep{nullptr, 0u, -1.});  // every voxel
  return LSA_OK;
}

// the two launches over n points at `src` (device), in the world already or moved there by m
int insert_device_points(lsa_dense_map* dm, const lsa_point_t* src, int n, const FrameMove& m, int frame, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  int rc = make_room(dm, n, who);
  if (rc) return rc;
  rc = scratch_room(ctx, &dm->slot_of, (int**)nullptr, &dm->slot_cap, (size_t)n, 4096);
  if (rc) return rc;
  const unsigned serial = dm->next_serial++;
  const float4* in = reinterpret_cast<const float4*>(src);
  const dim3 grid((n + 255) / 256);
  {
    ProfScope ps(ctx, "dense_claim", (double)n * 56, dm->stream);  // 32 B read, 4 B slot index, 20 B of atomic words
    hipLaunchKernelGGL(k_dense_claim, grid, dim3(256), 0, dm->stream, in, n, m, dm->leaf, table_of(dm), dm->stat, dm->slot_of);
  }
  {
    ProfScope ps(ctx, "dense_apply", (double)n * 12, dm->stream);
    hipLaunchKernelGGL(k_dense_apply, grid, dim3(256), 0, dm->stream, in, n, m, table_of(dm), dm->slot_of, frame, dm->stat, dm->host_words, serial);
  }
  dm->pending.emplace_back(serial, n);
  dm->pending_sum += n;
  dm->last_frame = frame;
  return LSA_OK;
}

int carve_ordinal(lsa_dense_map* dm, int frame, const char* who)
{
  if (frame < dm->last_frame) return dm->ctx->fail(LSA_E_ARG, std::string(who) + ": frame ordinals must not decrease");
  if (frame == INT32_MIN) return dm->ctx->fail(LSA_E_ARG, std::string(who) + ": the ordinal -2^31 is not carved (its word is the one for \"none\")");
  // (the default range under a leaf so small that lsa_dense_map_set would have refused it)
  if (!(dm->carve_range / dm->leaf <= kMaxRangeLeaves)) return dm->ctx->fail(LSA_E_ARG, std::string(who) + ": CarveRange is more than 4096 leaves");
  return LSA_OK;
}

// one launch over the rays of n points at `src` (device): every "CarveStride"-th point's, from origins (device, unfused) or
// from the frame's own origin under the point's pose (fused).  The first carve of a map makes its miss array.
int carve_device_points(lsa_dense_map* dm, const lsa_point_t* src, int n, const FrameMove& m, const float* origins, int n_origins, int frame, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  if (!dm->slots)
  {
    if (const int rc = make_room(dm, 0, who)) return rc;  // an empty table: the rays are counted all the same
  }
  if (!dm->miss)
  {
    const size_t bytes = (size_t)dm->capacity * 2 * sizeof(unsigned);
    if (hipMalloc((void**)&dm->miss, bytes) != hipSuccess)
    {
      (void)hipGetLastError();
      dm->miss = nullptr;
      return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory for " + std::to_string(bytes) + " bytes of misses; nothing was carved");
    }
    LSA_HIP(ctx, hipMemsetAsync(dm->miss, 0, bytes, dm->stream));
  }
  Carve c{};
  c.origins = origins;
  c.n_origins = n_origins;
  c.stride = dm->carve_stride;
  c.rays = (int)(((long long)n + c.stride - 1) / c.stride);
  c.frame = frame;
  c.leaf = dm->leaf;
  c.margin = dm->carve_margin_leaves * dm->leaf;
  c.range = dm->carve_range;
  c.max_steps = 3ll * ((long long)std::ceil(dm->carve_range / dm->leaf) + 2ll);
  {
    // per ray 32 B (and 12 B of origin) read; per visited voxel an 8-byte key at least -- not known here
    ProfScope ps(ctx, "dense_carve", (double)c.rays * 44, dm->stream);
    hipLaunchKernelGGL(k_dense_carve, dim3((c.rays + 255) / 256), dim3(256), 0, dm->stream, reinterpret_cast<const float4*>(src), m, c, table_of(dm), dm->stat);
  }
  dm->last_frame = frame;
  return LSA_OK;
}

}  // namespace

// waits for the insertions in flight; a probe sequence that ran out is reported here
int lsa::dense::settle(lsa_dense_map* dm, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  if (__atomic_load_n(&dm->host_words[1], __ATOMIC_ACQUIRE) != 0ull)
    return ctx->fail(LSA_E_STATE, std::string(who) + ": a probe sequence ran through the whole table (the map is incomplete; lsa_dense_map_clear starts again)");
  return LSA_OK;
}

double lsa::dense::now_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

namespace
{
Keep keep_of(const lsa_dense_map* dm, int min_frames, double max_miss_ratio) { return Keep{dm->miss, (unsigned)std::max(min_frames, 0), max_miss_ratio}; }

// keys and slot indices of the voxels that pass, in slot order, left in dm->keys[0] / index[0]; returns their number.  The
// map must be settled.
int compact_kept(lsa_dense_map* dm, int min_frames, double max_miss_ratio)
{
  lsa_ctx* ctx = dm->ctx;
  const int occupied = (int)occupied_bound(dm);  // exact: everything enqueued has been published
  if (occupied <= 0 || !dm->slots) return 0;
  const int nchunks = (int)((dm->capacity + 1023u) / 1024u);
  if (const int rc = scratch_room(ctx, &dm->chunks, (int**)nullptr, &dm->chunks_cap, (size_t)nchunks, 64)) return rc;
  if (occupied > dm->keys_cap)
  {
    for (int b = 0; b < 2; ++b) { retire_dev(ctx, dm->keys[b]); retire_dev(ctx, dm->index[b]); dm->keys[b] = nullptr; dm->index[b] = nullptr; }
    dm->keys_cap = 0;
    const size_t want = (size_t)occupied + (size_t)occupied / 2;
    for (int b = 0; b < 2; ++b)
    {
      LSA_HIP(ctx, hipMalloc((void**)&dm->keys[b], want * sizeof(u64)));
      LSA_HIP(ctx, hipMalloc((void**)&dm->index[b], want * sizeof(unsigned)));
    }
    dm->keys_cap = (int)want;
  }
  const Slot* slots = dm->slots;
  stable_compact(dm->stream, dm->chunks, dm->totals + 1, ExportPred{slots, keep_of(dm, min_frames, max_miss_ratio)}, ExportEmit{slots, dm->keys[0], dm->index[0]},
                 (const int*)nullptr, (int)dm->capacity, dm->totals);
  int kept = 0;
  LSA_HIP(ctx, hipMemcpyAsync(&kept, dm->totals, sizeof(int), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  return std::max(kept, 0);
}

// the voxels that pass (Keep) in ascending key order, left in dm->out_pts / out_vox / out_src / out_miss; returns their number
int export_sorted(lsa_dense_map* dm, int min_frames, double max_miss_ratio, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  const int rc = settle(dm, who);
  if (rc) return rc;
  const int kept = compact_kept(dm, min_frames, max_miss_ratio);
  if (kept <= 0) return kept;
  const Slot* slots = dm->slots;
  size_t tmp_bytes = 0;
  LSA_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, dm->keys[0], dm->keys[1], dm->index[0], dm->index[1], (size_t)kept, 0u, 63u, dm->stream));
  if (tmp_bytes > dm->sort_tmp_cap)
  {
    retire_dev(ctx, dm->sort_tmp);
    dm->sort_tmp = nullptr;
    dm->sort_tmp_cap = 0;
    LSA_HIP(ctx, hipMalloc(&dm->sort_tmp, tmp_bytes));
    dm->sort_tmp_cap = tmp_bytes;
  }
  LSA_HIP(ctx, rocprim::radix_sort_pairs(dm->sort_tmp, tmp_bytes, dm->keys[0], dm->keys[1], dm->index[0], dm->index[1], (size_t)kept, 0u, 63u, dm->stream));
  if (kept > dm->out_cap)
  {
    retire_dev(ctx, dm->out_pts);
    retire_dev(ctx, dm->out_vox);
    retire_dev(ctx, dm->out_src);
    retire_dev(ctx, dm->out_miss);
    dm->out_pts = nullptr; dm->out_vox = nullptr; dm->out_src = nullptr; dm->out_miss = nullptr; dm->out_cap = 0;
    const size_t want = (size_t)kept + (size_t)kept / 2;
    LSA_HIP(ctx, hipMalloc((void**)&dm->out_pts, want * sizeof(lsa_point_t)));
    LSA_HIP(ctx, hipMalloc((void**)&dm->out_vox, want * sizeof(lsa_dense_voxel_t)));
    LSA_HIP(ctx, hipMalloc((void**)&dm->out_src, want * sizeof(int)));
    LSA_HIP(ctx, hipMalloc((void**)&dm->out_miss, want * sizeof(unsigned)));
    dm->out_cap = (int)want;
  }
  hipLaunchKernelGGL(k_dense_gather, dim3((kept + 255) / 256), dim3(256), 0, dm->stream, slots, dm->source, dm->miss, dm->keys[1], dm->index[1], kept,
                     reinterpret_cast<float4*>(dm->out_pts), dm->out_vox, dm->out_src, dm->out_miss);
  return kept;
}

// the records of the voxels that pass, in ascending key order, left in dm->out_normals behind export_sorted's points; returns
// their number.  A refusal comes before anything is waited for.
int normals_sorted(lsa_dense_map* dm, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors, const float* viewpoints_xyz, int n_viewpoints,
                   int first_frame, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  if (radius_leaves != 1 && radius_leaves != 2) return ctx->fail(LSA_E_ARG, std::string(who) + ": radius_leaves is 1 or 2");
  const int side = 2 * radius_leaves + 1;
  if (min_neighbors < 3 || min_neighbors > side * side * side) return ctx->fail(LSA_E_ARG, std::string(who) + ": min_neighbors between 3 and (2 * radius_leaves + 1)^3");
  if (min_frames < 1) return ctx->fail(LSA_E_ARG, std::string(who) + ": min_frames >= 1");
  if (n_viewpoints < 0 || (n_viewpoints > 0 && !viewpoints_xyz)) return ctx->fail(LSA_E_ARG, std::string(who) + ": viewpoints are n_viewpoints x 3 floats");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  if (n_viewpoints > 0)
  {
    if (const int rc = scratch_room(ctx, &dm->viewpoints, (float**)nullptr, &dm->viewpoints_cap, (size_t)n_viewpoints * 3, 3 * 256)) return rc;
    LSA_HIP(ctx, hipMemcpyAsync(dm->viewpoints, viewpoints_xyz, (size_t)n_viewpoints * 3 * sizeof(float), hipMemcpyHostToDevice, dm->stream));
    LSA_HIP(ctx, hipStreamSynchronize(dm->stream));  // may be pageable and reused by the caller
  }
  const int kept = export_sorted(dm, min_frames, max_miss_ratio, who);
  if (kept <= 0) return kept;
  if (const int rc = scratch_room(ctx, &dm->out_normals, (unsigned**)nullptr, &dm->out_normals_cap, (size_t)kept * 5, 5 * 4096)) return rc;
  if (const int rc = scratch_room(ctx, &dm->normal_sums, (double**)nullptr, &dm->normal_sums_cap, (size_t)kept * 9, 9 * 4096)) return rc;
  Normals c{};
  c.keys = dm->keys[1];
  c.index = dm->index[1];
  c.n = kept;
  c.r = radius_leaves;
  c.min_neighbors = (unsigned)min_neighbors;
  c.viewpoints = n_viewpoints > 0 ? dm->viewpoints : nullptr;
  c.n_viewpoints = n_viewpoints;
  c.first_frame = first_frame;
  c.keep = keep_of(dm, min_frames, max_miss_ratio);
  {
    // per voxel its key, slot, 20 B of record and 2 x 72 B of sums; per cell a key at least, per neighbour 16 B of point -- not known here
    ProfScope ps(ctx, "dense_normals", (double)kept * (176 + 8. * side * side * side), dm->stream);
    hipLaunchKernelGGL(k_dense_normals, dim3((kept + kNormalGroups - 1) / kNormalGroups), dim3(kNormalLanes * kNormalGroups), 0, dm->stream, c, table_of(dm), dm->normal_sums,
                       dm->out_normals);
    hipLaunchKernelGGL(k_dense_normal_records, dim3((kept + 255) / 256), dim3(256), 0, dm->stream, c, table_of(dm), dm->normal_sums, dm->out_normals);
  }
  LSA_HIP(ctx, hipGetLastError());
  return kept;
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
  if (bytes > dm->grid_scratch_cap)
  {
    retire_dev(ctx, dm->grid_scratch);
    dm->grid_scratch = nullptr;
    dm->grid_scratch_cap = 0;
    const size_t want = bytes + bytes / 4;
    if (hipMalloc((void**)&dm->grid_scratch, want) != hipSuccess)
    {
      (void)hipGetLastError();
      dm->grid_scratch = nullptr;
      return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory for " + std::to_string(want) + " bytes of rasters; ask for a smaller window");
    }
    dm->grid_scratch_cap = want;
  }
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

int lsa_dense_map_create(lsa_ctx* ctx, double leaf, lsa_dense_map** out)
{
  if (!ctx || !out) return ctx ? ctx->fail(LSA_E_ARG, "lsa_dense_map_create: bad argument") : LSA_E_ARG;
  *out = nullptr;
  if (!(leaf > 0.) || !std::isfinite(leaf)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_create: the leaf size must be positive and finite");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  lsa_dense_map* dm = new lsa_dense_map;
  dm->ctx = ctx;
  dm->stream = ctx->prefetch_stream;  // beside the next frame's registration, with the rolling maps' kernels: no fourth stream
  dm->leaf = leaf;
  bool ok = hipMalloc((void**)&dm->stat, kStatWords * sizeof(u64)) == hipSuccess;
  ok = ok && hipMemset(dm->stat, 0, kStatWords * sizeof(u64)) == hipSuccess;
  ok = ok && hipMalloc((void**)&dm->totals, 2 * sizeof(int)) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&dm->host_words, 4 * sizeof(u64), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess;
  ok = ok && hipEventCreateWithFlags(&dm->ev_frame, hipEventDisableTiming) == hipSuccess;
  if (ok && !ctx->ev_dense) ok = hipEventCreateWithFlags(&ctx->ev_dense, hipEventDisableTiming) == hipSuccess;
  if (!ok)
  {
    (void)hipGetLastError();
    lsa_dense_map_destroy(dm);
    return ctx->fail(LSA_E_HIP, "lsa_dense_map_create: allocation failed");
  }
  std::memset(dm->host_words, 0, 4 * sizeof(u64));
  *out = dm;
  return LSA_OK;
}

void lsa_dense_map_destroy(lsa_dense_map* dm)
{
  if (!dm) return;
  (void)hipSetDevice(dm->ctx->device);
  if (dm->stream) (void)hipStreamSynchronize(dm->stream);
  auto fr = [](void* p) { if (p) (void)hipFree(p); };
  fr(dm->slots); fr(dm->source); fr(dm->miss); fr(dm->staged_origins); fr(dm->out_miss); fr(dm->stat); fr(dm->slot_of); fr(dm->staged); fr(dm->chunks); fr(dm->totals);
  for (int b = 0; b < 2; ++b) { fr(dm->keys[b]); fr(dm->index[b]); }
  fr(dm->grid_scratch); fr(dm->grid_box); fr(dm->cast_scratch);
  fr(dm->viewpoints); fr(dm->out_normals); fr(dm->normal_sums); fr(dm->sort_tmp); fr(dm->out_pts); fr(dm->out_vox); fr(dm->out_src);
  if (dm->host_words) (void)hipHostFree(dm->host_words);
  if (dm->ev_frame) (void)hipEventDestroy(dm->ev_frame);
  delete dm;
}

int lsa_dense_map_set(lsa_dense_map* dm, const char* name, double value)
{
  if (!dm || !name) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const std::string n(name);
  if (n == "MaxBytes")
  {
    if (!(value >= 0.)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_set: MaxBytes >= 0 (0: no limit)");
    dm->max_bytes = (size_t)value;
    return LSA_OK;
  }
  if (n == "InitialCapacity")
  {
    if (!(value >= 1.) || value > (double)kMaxCapacity) return ctx->fail(LSA_E_ARG, "lsa_dense_map_set: InitialCapacity between 1 and 2^30 slots");
    unsigned cap = kMinCapacity;
    while ((double)cap < value) cap *= 2;
    dm->initial_capacity = cap;  // of the table the next insertion into a map without one makes
    return LSA_OK;
  }
  if (n == "ProbeStress")
  {
    // a TEST KNOB: every key's home slot is 0, so that probe sequences are as long as the table is full
    if (dm->slots && ((value != 0.) != (dm->stress != 0)))
    {
      const int rc = settle(dm, "lsa_dense_map_set");
      if (rc) return rc;
      if (occupied_bound(dm) > 0) return ctx->fail(LSA_E_STATE, "lsa_dense_map_set: ProbeStress only on an empty map");
    }
    dm->stress = value != 0. ? 1 : 0;
    return LSA_OK;
  }
  if (n == "CarveMarginLeaves")
  {
    if (!(value >= 0.) || !std::isfinite(value)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_set: CarveMarginLeaves >= 0");
    dm->carve_margin_leaves = value;
    return LSA_OK;
  }
  if (n == "CarveRange")
  {
    // the bound of every ray's walk: 3 * (CarveRange / leaf + 2) steps
    if (!(value > 0.) || !(value / dm->leaf <= kMaxRangeLeaves)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_set: CarveRange positive and at most 4096 leaves");
    dm->carve_range = value;
    return LSA_OK;
  }
  if (n == "CarveStride")
  {
    if (!(value >= 1.) || value > 1e9 || value != std::floor(value)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_set: CarveStride a whole number >= 1");
    dm->carve_stride = (int)value;
    return LSA_OK;
  }
  if (n == "GridMaxCells")
  {
    // the most cells lsa_dense_map_get_grid hands out in one call
    if (!(value >= 1.) || value > (double)(1ll << 28) || value != std::floor(value)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_set: GridMaxCells a whole number between 1 and 2^28");
    dm->grid_max_cells = (long long)value;
    return LSA_OK;
  }
  return ctx->fail(LSA_E_ARG, "lsa_dense_map_set: unknown parameter " + n);
}

double lsa_dense_map_get_param(lsa_dense_map* dm, const char* name)
{
  if (!dm || !name) return -1.;
  const std::string n(name);
  if (n == "LeafSize") return dm->leaf;
  if (n == "MaxBytes") return (double)dm->max_bytes;
  if (n == "InitialCapacity") return dm->initial_capacity;
  if (n == "ProbeStress") return dm->stress;
  if (n == "Capacity") return dm->capacity;
  if (n == "Rehashes") return dm->rehashes;
  if (n == "ExportSeconds") return dm->export_seconds;
  if (n == "Reprojections") return dm->reprojections;
  if (n == "Dropped") return (double)dm->dropped;
  if (n == "ReprojectSeconds") return dm->reproject_seconds;
  if (n == "CarveMarginLeaves") return dm->carve_margin_leaves;
  if (n == "CarveRange") return dm->carve_range;
  if (n == "CarveStride") return dm->carve_stride;
  if (n == "CarveSeconds") return dm->carve_seconds;
  if (n == "Pruned") return (double)dm->pruned;
  if (n == "Prunes") return dm->prunes;
  if (n == "NormalsSeconds") return dm->normals_seconds;
  if (n == "GridMaxCells") return (double)dm->grid_max_cells;
  if (n == "GridSeconds") return dm->grid_seconds;
  if (n == "Rays")
  {
    // the device's word, behind the carves in flight
    u64 rays = 0;
    if (settle(dm, "lsa_dense_map_get_param") != LSA_OK) return -1.;
    if (hipMemcpy(&rays, dm->stat + kStatRays, sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) return -1.;
    return (double)rays;
  }
  if (n == "CastSeconds") return dm->cast_seconds;
  if (n == "CastRays")
  {
    // the rays of lsa_dense_map_cast and _compare_* since the last clear (lsa_dense_cast.hip): a word of their own, not "Rays"
    u64 rays = 0;
    if (settle(dm, "lsa_dense_map_get_param") != LSA_OK) return -1.;
    if (hipMemcpy(&rays, dm->stat + kStatCastRays, sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) return -1.;
    return (double)rays;
  }
  return -1.;
}

int lsa_dense_map_insert_points(lsa_dense_map* dm, const lsa_point_t* pts, int n, int frame)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  if (n < 0 || (n > 0 && !pts)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_insert_points: bad argument");
  if (frame < dm->last_frame) return ctx->fail(LSA_E_ARG, "lsa_dense_map_insert_points: frame ordinals must not decrease");
  if (n == 0) { dm->last_frame = frame; return LSA_OK; }
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = make_room(dm, n, "lsa_dense_map_insert_points");  // a refusal comes before anything is touched
  if (rc) return rc;
  rc = scratch_room(ctx, &dm->staged, (lsa_point_t**)nullptr, &dm->staged_cap, (size_t)n, 4096);
  if (rc) return rc;
  LSA_HIP(ctx, hipMemcpyAsync(dm->staged, pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyHostToDevice, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));  // pts may be pageable and reused by the caller
  FrameMove m{};
  return insert_device_points(dm, dm->staged, n, m, frame, "lsa_dense_map_insert_points");
}

int lsa_dense_map_insert_frame(lsa_dense_map* dm, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset, int frame)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  if (!H0 || (interpolate && !H1)) return ctx->fail(LSA_E_ARG, "lsa_dense_map_insert_frame: bad argument");
  if (!ctx->frame || ctx->frame_n <= 0) return ctx->fail(LSA_E_STATE, "lsa_dense_map_insert_frame: no frame");
  if (frame < dm->last_frame) return ctx->fail(LSA_E_ARG, "lsa_dense_map_insert_frame: frame ordinals must not decrease");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const int n = ctx->frame_n;
  FrameMove m{};
  m.fused = 1;
  m.interpolate = interpolate ? 1 : 0;
  row_major_to_rt(H0, m.R.R, m.R.t);
  if (interpolate) m.c = make_interp_const(H0, H1, t0, t1);
  m.time_offset = time_offset;
  // the frame is whatever the context's stream has made of it so far (upload, times from the advancement); the buffer is
  // then held until the insertion is over by an event its next writer waits for (frame_writer_guard), never by the host
  LSA_HIP(ctx, hipEventRecord(dm->ev_frame, ctx->stream));
  LSA_HIP(ctx, hipStreamWaitEvent(dm->stream, dm->ev_frame, 0));
  // (a refusal comes from make_room, before anything is touched)
  const int rc = insert_device_points(dm, ctx->frame, n, m, frame, "lsa_dense_map_insert_frame");
  if (rc) return rc;
  LSA_HIP(ctx, hipEventRecord(ctx->ev_dense, dm->stream));
  ctx->dense_frame_pending = true;
  return LSA_OK;
}

int lsa_dense_map_carve_points(lsa_dense_map* dm, const lsa_point_t* pts, int n, const float* origins_xyz, int n_origins, int frame)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_carve_points";
  if (n < 0 || (n > 0 && (!pts || !origins_xyz)) || (n > 0 && n_origins != 1 && n_origins != n)) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument (one origin, or one per point)");
  if (const int rc = carve_ordinal(dm, frame, who)) return rc;
  if (n == 0) { dm->last_frame = frame; return LSA_OK; }
  const double t0 = now_seconds();
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = scratch_room(ctx, &dm->staged, (lsa_point_t**)nullptr, &dm->staged_cap, (size_t)n, 4096);
  if (rc) return rc;
  rc = scratch_room(ctx, &dm->staged_origins, (float**)nullptr, &dm->staged_origins_cap, (size_t)n_origins * 3, 3 * 4096);
  if (rc) return rc;
  LSA_HIP(ctx, hipMemcpyAsync(dm->staged, pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyHostToDevice, dm->stream));
  LSA_HIP(ctx, hipMemcpyAsync(dm->staged_origins, origins_xyz, (size_t)n_origins * 3 * sizeof(float), hipMemcpyHostToDevice, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));  // both may be pageable and reused by the caller
  FrameMove m{};
  rc = carve_device_points(dm, dm->staged, n, m, dm->staged_origins, n_origins, frame, who);
  dm->carve_seconds = now_seconds() - t0;
  return rc;
}

int lsa_dense_map_carve_frame(lsa_dense_map* dm, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset, int frame)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_carve_frame";
  if (!H0 || (interpolate && !H1)) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  if (!ctx->frame || ctx->frame_n <= 0) return ctx->fail(LSA_E_STATE, std::string(who) + ": no frame");
  if (const int rc = carve_ordinal(dm, frame, who)) return rc;
  const double started = now_seconds();
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  FrameMove m{};
  m.fused = 1;
  m.interpolate = interpolate ? 1 : 0;
  row_major_to_rt(H0, m.R.R, m.R.t);
  if (interpolate) m.c = make_interp_const(H0, H1, t0, t1);
  m.time_offset = time_offset;
  // as the fused insertion: the frame as the context's stream has left it, held by an event its next writer waits for --
  // recorded behind the carve, which reads the buffer last
  LSA_HIP(ctx, hipEventRecord(dm->ev_frame, ctx->stream));
  LSA_HIP(ctx, hipStreamWaitEvent(dm->stream, dm->ev_frame, 0));
  const int rc = carve_device_points(dm, ctx->frame, ctx->frame_n, m, nullptr, 0, frame, who);
  if (rc) return rc;
  LSA_HIP(ctx, hipEventRecord(ctx->ev_dense, dm->stream));
  ctx->dense_frame_pending = true;
  dm->carve_seconds = now_seconds() - started;
  return LSA_OK;
}

int lsa_dense_map_prune(lsa_dense_map* dm, int min_frames, double max_miss_ratio, long long* removed)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_prune";
  if (!removed) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  *removed = 0;
  int rc = settle(dm, who);
  if (rc) return rc;
  const long long occupied = occupied_bound(dm);  // exact after settle
  dm->prunes++;
  if (!dm->slots || occupied <= 0) return LSA_OK;
  const int kept = compact_kept(dm, min_frames, max_miss_ratio);
  if (kept < 0) return kept;
  if (kept == occupied) return LSA_OK;  // nothing to remove: the table stays
  unsigned cap = kMinCapacity;
  while ((long long)(cap / 2) < (long long)kept) cap *= 2;  // kept <= occupied <= capacity / 2: never above the table's own
  Slot* fresh = nullptr;
  int* fresh_source = nullptr;
  unsigned* fresh_miss = nullptr;
  rc = fresh_table(dm, cap, &fresh, &fresh_source, &fresh_miss, who, "the map is as it was");
  if (rc) return rc;
  const Keep keep = keep_of(dm, min_frames, max_miss_ratio);  // reads the old miss array
  rehash_into(dm, fresh, fresh_source, fresh_miss, cap, keep);
  const unsigned serial = dm->next_serial++;
  hipLaunchKernelGGL(k_dense_publish, dim3(1), dim3(64), 0, dm->stream, dm->stat, dm->host_words, serial, (unsigned)kept);
  LSA_HIP(ctx, hipGetLastError());
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  dm->seen_serial = serial;
  dm->known = (unsigned)kept;
  dm->pending.clear();
  dm->pending_sum = 0;
  *removed = occupied - kept;
  dm->pruned += *removed;
  if (__atomic_load_n(&dm->host_words[1], __ATOMIC_ACQUIRE) != 0ull)
    return ctx->fail(LSA_E_STATE, std::string(who) + ": a probe sequence ran through the whole table (the map is incomplete; lsa_dense_map_clear starts again)");
  return LSA_OK;
}

int lsa_dense_map_reserve(lsa_dense_map* dm, long long n)
{
  if (!dm) return LSA_E_ARG;
  if (n < 0) return dm->ctx->fail(LSA_E_ARG, "lsa_dense_map_reserve: bad argument");
  if (hipSetDevice(dm->ctx->device) != hipSuccess) return dm->ctx->fail(LSA_E_HIP, "lsa_dense_map_reserve: hipSetDevice");
  return make_room(dm, n, "lsa_dense_map_reserve");
}

int lsa_dense_map_size(lsa_dense_map* dm)
{
  if (!dm) return LSA_E_ARG;
  const int rc = settle(dm, "lsa_dense_map_size");
  return rc ? rc : (int)occupied_bound(dm);
}

long long lsa_dense_map_skipped(lsa_dense_map* dm)
{
  if (!dm) return LSA_E_ARG;
  const int rc = settle(dm, "lsa_dense_map_skipped");
  if (rc) return rc;
  return dm->seen_serial >= dm->epoch ? (long long)__atomic_load_n(&dm->host_words[2], __ATOMIC_ACQUIRE) : 0ll;
}

long long lsa_dense_map_bytes(const lsa_dense_map* dm)
{
  if (!dm) return LSA_E_ARG;
  return (long long)dm->capacity * (long long)(sizeof(Slot) + sizeof(int) + (dm->miss ? 2 * sizeof(unsigned) : 0)) + (long long)dm->slot_cap * (long long)sizeof(int);
}

int lsa_dense_map_get(lsa_dense_map* dm, int min_frames, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity)
{
  return lsa_dense_map_get_filtered(dm, min_frames, -1., pts, voxels, capacity);
}

int lsa_dense_map_get_filtered(lsa_dense_map* dm, int min_frames, double max_miss_ratio, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  if (capacity < 0) return ctx->fail(LSA_E_ARG, "lsa_dense_map_get: bad argument");
  const double t0 = now_seconds();
  const int kept = export_sorted(dm, min_frames, max_miss_ratio, "lsa_dense_map_get");
  if (kept <= 0) return kept;
  const int n = std::min(kept, capacity);
  if (n > 0 && pts) LSA_HIP(ctx, hipMemcpyAsync(pts, dm->out_pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyDeviceToHost, dm->stream));
  if (n > 0 && voxels) LSA_HIP(ctx, hipMemcpyAsync(voxels, dm->out_vox, (size_t)n * sizeof(lsa_dense_voxel_t), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  dm->export_seconds = now_seconds() - t0;
  return kept;
}

int lsa_dense_map_get_sources(lsa_dense_map* dm, int min_frames, int* out, int capacity)
{
  return lsa_dense_map_get_sources_filtered(dm, min_frames, -1., out, capacity);
}

int lsa_dense_map_get_misses(lsa_dense_map* dm, int min_frames, double max_miss_ratio, uint32_t* out, int capacity)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  if (capacity < 0) return ctx->fail(LSA_E_ARG, "lsa_dense_map_get_misses: bad argument");
  const int kept = export_sorted(dm, min_frames, max_miss_ratio, "lsa_dense_map_get_misses");
  if (kept <= 0) return kept;
  const int n = std::min(kept, capacity);
  if (n > 0 && out) LSA_HIP(ctx, hipMemcpyAsync(out, dm->out_miss, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  return kept;
}

int lsa_dense_map_get_sources_filtered(lsa_dense_map* dm, int min_frames, double max_miss_ratio, int* out, int capacity)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  if (capacity < 0) return ctx->fail(LSA_E_ARG, "lsa_dense_map_get_sources: bad argument");
  const int kept = export_sorted(dm, min_frames, max_miss_ratio, "lsa_dense_map_get_sources");
  if (kept <= 0) return kept;
  const int n = std::min(kept, capacity);
  if (n > 0 && out) LSA_HIP(ctx, hipMemcpyAsync(out, dm->out_src, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  return kept;
}

int lsa_dense_map_get_normals(lsa_dense_map* dm, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors, const float* viewpoints_xyz,
                              int n_viewpoints, int first_frame, lsa_dense_normal_t* out, int capacity)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_get_normals";
  if (capacity < 0) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  const double t0 = now_seconds();
  const int kept = normals_sorted(dm, min_frames, max_miss_ratio, radius_leaves, min_neighbors, viewpoints_xyz, n_viewpoints, first_frame, who);
  if (kept <= 0) return kept;
  const int n = std::min(kept, capacity);
  if (n > 0 && out) LSA_HIP(ctx, hipMemcpyAsync(out, dm->out_normals, (size_t)n * sizeof(lsa_dense_normal_t), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  dm->normals_seconds = now_seconds() - t0;
  return kept;
}

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

int lsa_dense_map_reproject(lsa_dense_map* dm, const double* corrections16, int first_frame, int n, long long* dropped)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_reproject";
  if (!corrections16 || !dropped || n < 1) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  int rc = settle(dm, who);
  if (rc) return rc;
  const double t0 = now_seconds();
  *dropped = 0;
  if (!dm->slots || occupied_bound(dm) <= 0)  // exact after settle: an empty map has nothing to move
  {
    dm->reprojections++;
    dm->reproject_seconds = now_seconds() - t0;
    return LSA_OK;
  }
  const unsigned cap = dm->capacity;
  // everything that needs memory comes first: a refusal leaves the map as it was
  const size_t corrections_bytes = (size_t)n * 16 * sizeof(double);
  const size_t scratch_bytes = (size_t)cap * (2 * sizeof(u64) + sizeof(int));  // pick, frames, to
  double* corrections = nullptr;
  unsigned char* scratch = nullptr;
  if (hipMalloc((void**)&corrections, corrections_bytes) != hipSuccess || hipMalloc((void**)&scratch, scratch_bytes) != hipSuccess)
  {
    (void)hipGetLastError();
    if (corrections) (void)hipFree(corrections);
    return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory for " + std::to_string(corrections_bytes + scratch_bytes) + " bytes of corrections and scratch; the map is as it was");
  }
  Slot* fresh = nullptr;
  int* fresh_source = nullptr;
  unsigned* fresh_miss = nullptr;
  rc = fresh_table(dm, cap, &fresh, &fresh_source, &fresh_miss, who, "the map is as it was");
  if (rc)
  {
    (void)hipFree(corrections);
    (void)hipFree(scratch);
    return rc;
  }
  Reproject r;
  r.old = dm->slots;
  r.old_source = dm->source;
  r.old_miss = fresh_miss ? dm->miss : nullptr;
  r.old_capacity = cap;
  r.corrections = corrections;
  r.first_frame = first_frame;
  r.n = n;
  r.leaf = dm->leaf;
  r.pick = reinterpret_cast<u64*>(scratch);
  r.frames = r.pick + cap;
  r.to = reinterpret_cast<int*>(r.frames + cap);
  // from here on the old table belongs to the graveyard and the new one is the map's, whatever a launch answers
  Slot* old = dm->slots;
  int* old_source = dm->source;
  unsigned* old_miss = fresh_miss ? dm->miss : nullptr;
  dm->slots = fresh;
  dm->source = fresh_source;
  if (fresh_miss) dm->miss = fresh_miss;
  const Table t = table_of(dm);
  const unsigned serial = dm->next_serial++;
  const dim3 grid((cap + 255) / 256);
  hipError_t e = hipMemcpyAsync(corrections, corrections16, corrections_bytes, hipMemcpyHostToDevice, dm->stream);
  if (e == hipSuccess) e = hipMemsetAsync(r.pick, 0xff, (size_t)cap * sizeof(u64), dm->stream);
  if (e == hipSuccess) e = hipMemsetAsync(r.frames, 0, (size_t)cap * sizeof(u64), dm->stream);
  // the new table counts its own slots; error and skipped go on
  if (e == hipSuccess) e = hipMemsetAsync(&dm->stat[kStatOccupied], 0, sizeof(u64), dm->stream);
  if (e == hipSuccess) e = hipMemsetAsync(&dm->stat[kStatDropped], 0, sizeof(u64), dm->stream);
  if (e == hipSuccess)
  {
    {
      // per old slot 4 B of `to`; per voxel 68 B read, the correction, 8 B of key CAS and 28 B of atomic words
      ProfScope ps(ctx, "dense_move", (double)cap * 4 + (double)dm->known * 104, dm->stream);
      hipLaunchKernelGGL(k_dense_move, grid, dim3(256), 0, dm->stream, r, t, dm->stat);
    }
    {
      ProfScope ps(ctx, "dense_elect", (double)cap * 4 + (double)dm->known * 84, dm->stream);
      hipLaunchKernelGGL(k_dense_elect, grid, dim3(256), 0, dm->stream, r, t);
    }
    {
      ProfScope ps(ctx, "dense_settle", (double)cap * 4 + (double)dm->known * 160, dm->stream);
      hipLaunchKernelGGL(k_dense_settle, grid, dim3(256), 0, dm->stream, r, t, dm->stat, dm->host_words, serial);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(dm->stream);  // the count of the dropped is the call's answer
  retire_dev(ctx, old);
  retire_dev(ctx, old_source);
  retire_dev(ctx, old_miss);
  retire_dev(ctx, corrections);
  retire_dev(ctx, scratch);
  if (e != hipSuccess) return ctx->fail(LSA_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  // everything enqueued has been published: the bound of the occupied slots is the new table's count
  const u64 w = __atomic_load_n(&dm->host_words[0], __ATOMIC_ACQUIRE);
  dm->seen_serial = serial;
  dm->known = (unsigned)w;
  dm->pending.clear();
  dm->pending_sum = 0;
  *dropped = (long long)__atomic_load_n(&dm->host_words[3], __ATOMIC_ACQUIRE);
  dm->dropped += *dropped;
  dm->reprojections++;
  dm->reproject_seconds = now_seconds() - t0;
  if (__atomic_load_n(&dm->host_words[1], __ATOMIC_ACQUIRE) != 0ull)
    return ctx->fail(LSA_E_STATE, std::string(who) + ": a probe sequence ran through the whole table (the map is incomplete; lsa_dense_map_clear starts again)");
  return LSA_OK;
}

int lsa_dense_map_clear(lsa_dense_map* dm)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  if (dm->slots) LSA_HIP(ctx, hipMemsetAsync(dm->slots, 0, (size_t)dm->capacity * sizeof(Slot), dm->stream));
  if (dm->source) LSA_HIP(ctx, hipMemsetAsync(dm->source, 0, (size_t)dm->capacity * sizeof(int), dm->stream));
  if (dm->miss) LSA_HIP(ctx, hipMemsetAsync(dm->miss, 0, (size_t)dm->capacity * 2 * sizeof(unsigned), dm->stream));
  LSA_HIP(ctx, hipMemsetAsync(dm->stat, 0, kStatWords * sizeof(u64), dm->stream));
  // what insertions before the clear still publish is older than the epoch and ignored; the error word goes with them
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  dm->host_words[1] = 0ull;
  dm->epoch = dm->next_serial;
  dm->seen_serial = dm->epoch - 1u;
  dm->known = 0;
  dm->pending.clear();
  dm->pending_sum = 0;
  dm->last_frame = INT32_MIN;
  dm->dropped = 0;
  dm->pruned = 0;
  return LSA_OK;
}

int lsa_dense_map_save_pcd(lsa_dense_map* dm, const char* path, int format, int min_frames)
{
  return lsa_dense_map_save_pcd_filtered(dm, path, format, min_frames, -1.);
}

int lsa_dense_map_save_pcd_filtered(lsa_dense_map* dm, const char* path, int format, int min_frames, double max_miss_ratio)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  if (!path) return ctx->fail(LSA_E_ARG, "lsa_dense_map_save_pcd: no path");
  if (format < pcd::kAscii || format > pcd::kBinaryCompressed) return ctx->fail(-4, std::string(path) + ": unknown PCD format " + std::to_string(format));
  try
  {
    double* T = ctx->pcd_times;
    std::fill(T, T + 8, 0.);
    const double t0 = now_seconds();
    const int kept = export_sorted(dm, min_frames, max_miss_ratio, "lsa_dense_map_save_pcd");
    if (kept < 0) return kept;
    T[4] = now_seconds() - t0;
    return pcd_save_device_points(ctx, dm->stream, dm->out_pts, kept, path, format);
  }
  catch (const std::bad_alloc&) { return ctx->fail(LSA_E_CAPACITY, std::string(path) + ": not enough host memory"); }
}

int lsa_dense_map_save_pcd_normals(lsa_dense_map* dm, const char* path, int format, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors,
                                   const float* viewpoints_xyz, int n_viewpoints, int first_frame)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_save_pcd_normals";
  if (!path) return ctx->fail(LSA_E_ARG, std::string(who) + ": no path");
  if (format < pcd::kAscii || format > pcd::kBinaryCompressed) return ctx->fail(-4, std::string(path) + ": unknown PCD format " + std::to_string(format));
  try
  {
    double* T = ctx->pcd_times;
    std::fill(T, T + 8, 0.);
    const double t0 = now_seconds();
    const int kept = normals_sorted(dm, min_frames, max_miss_ratio, radius_leaves, min_neighbors, viewpoints_xyz, n_viewpoints, first_frame, who);
    if (kept <= 0) return kept;
    // the four floats of every record, for the writer to put behind the point (the path is not hot)
    std::vector<lsa_dense_normal_t> records((size_t)kept);
    LSA_HIP(ctx, hipMemcpyAsync(records.data(), dm->out_normals, (size_t)kept * sizeof(lsa_dense_normal_t), hipMemcpyDeviceToHost, dm->stream));
    LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
    std::vector<float> normals4((size_t)kept * 4);
    for (int i = 0; i < kept; ++i) std::memcpy(&normals4[(size_t)i * 4], &records[(size_t)i], 4 * sizeof(float));
    T[4] = now_seconds() - t0;
    return pcd_save_device_points(ctx, dm->stream, dm->out_pts, kept, path, format, normals4.data());
  }
  catch (const std::bad_alloc&) { return ctx->fail(LSA_E_CAPACITY, std::string(path) + ": not enough host memory"); }
}

}  // extern "C"
