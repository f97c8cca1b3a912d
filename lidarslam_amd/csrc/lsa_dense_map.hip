// lsa_dense_map.hip -- the dense point-cloud map: registered frames voxel-hashed on the device (the host
// statement the table is held to, byte for byte, is DenseMapHost in lidarslam_amd/_dense_map.py).  This unit is the table's
// life: insertion, growth, the prune, the parameters; what the units share -- the slot, the table, the map's host object -- is
// in lsa_dense_table.h, and DESIGN.md 3.14 says which unit holds what.
//
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
// table of twice the size on the same stream; the old table goes to the context's graveyard.  The miss array of a map that
// has been carved is carried by the rehash, and lsa_dense_map_prune is the rehash under the export's predicate into the
// smallest table that holds what passes.
#include <chrono>
#include <cmath>
#include <cstring>
#include "lsa_dense_table.h"
#include "lsa_device_math.h"

namespace lsa
{
InterpConst make_interp_const(const double H0[16], const double H1[16], double t0, double t1);  // lsa_transform.hip
}
using namespace lsa;
using namespace lsa::dense;

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
  add_once_a_wavefront(&stat[kStatSkipped], !ok);
  if (!ok)
  {
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

// launch 2: the winner of every voxel of the call applies the rule; one thread publishes the counts launch 1 has left final
__global__ __launch_bounds__(256) void k_dense_apply(const float4* __restrict__ in, int n, const FrameMove m, Table t, const int* __restrict__ slot_of, int frame,
                                                     const u64* __restrict__ stat, u64* __restrict__ host_words, unsigned serial)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) publish_counts(stat, host_words, serial, false);
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
  publish_counts(stat, host_words, serial, false);
}

// the table `fresh` of `cap` slots takes what `keep` lets through of the map's and becomes the map's
void rehash_into(lsa_dense_map* dm, const TableArrays& fresh, const Keep& keep)
{
  const TableArrays old = swap_table(dm, fresh);
  if (!old.slots) return;
  ProfScope ps(dm->ctx, "dense_rehash", (double)old.capacity * (sizeof(Slot) + sizeof(int)) * 2, dm->stream);
  hipLaunchKernelGGL(k_dense_rehash, dim3((old.capacity + 255) / 256), dim3(256), 0, dm->stream, old.slots, old.source, old.miss, old.capacity, keep, table_of(dm),
                     dm->stat);
  retire_dev(dm->ctx, old.slots);
  retire_dev(dm->ctx, old.source);
  retire_dev(dm->ctx, old.miss);
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
}  // namespace

double lsa::dense::now_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int lsa::dense::probe_ran_out(lsa_dense_map* dm, const char* who)
{
  if (__atomic_load_n(&dm->host_words[1], __ATOMIC_ACQUIRE) == 0ull) return LSA_OK;
  return dm->ctx->fail(LSA_E_STATE, std::string(who) + ": a probe sequence ran through the whole table (the map is incomplete; lsa_dense_map_clear starts again)");
}

int lsa::dense::settle(lsa_dense_map* dm, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  return probe_ran_out(dm, who);
}

long long lsa::dense::occupied_bound(lsa_dense_map* dm)
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

void* lsa::dense::fresh_zeroed(lsa_dense_map* dm, size_t bytes, hipError_t* e)
{
  void* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess)
  {
    (void)hipGetLastError();
    *e = hipErrorOutOfMemory;
    return nullptr;
  }
  *e = hipMemsetAsync(p, 0, bytes, dm->stream);
  if (*e == hipSuccess) return p;
  (void)hipStreamSynchronize(dm->stream);
  (void)hipFree(p);
  return nullptr;
}

int lsa::dense::fresh_table(lsa_dense_map* dm, unsigned cap, TableArrays* fresh, const char* who, const char* consequence)
{
  lsa_ctx* ctx = dm->ctx;
  const size_t bytes = (size_t)cap * sizeof(Slot), source_bytes = (size_t)cap * sizeof(int), miss_bytes = dm->miss ? (size_t)cap * 2 * sizeof(unsigned) : 0;
  hipError_t e = hipSuccess;
  fresh->capacity = cap;
  fresh->slots = static_cast<Slot*>(fresh_zeroed(dm, bytes, &e));
  fresh->source = fresh->slots ? static_cast<int*>(fresh_zeroed(dm, source_bytes, &e)) : nullptr;
  fresh->miss = fresh->source && miss_bytes ? static_cast<unsigned*>(fresh_zeroed(dm, miss_bytes, &e)) : nullptr;
  if (e == hipSuccess) return LSA_OK;
  (void)hipStreamSynchronize(dm->stream);  // the memsets of the arrays that came about: over before they are freed
  if (fresh->source) (void)hipFree(fresh->source);
  if (fresh->slots) (void)hipFree(fresh->slots);
  *fresh = TableArrays{};
  if (e != hipErrorOutOfMemory) return ctx->fail(LSA_E_HIP, std::string(who) + ": hipMemsetAsync: " + hipGetErrorString(e));
  return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory for a table of " + std::to_string(bytes + source_bytes + miss_bytes) + " bytes; " + consequence);
}

TableArrays lsa::dense::swap_table(lsa_dense_map* dm, const TableArrays& fresh)
{
  const TableArrays old{dm->slots, dm->source, fresh.miss ? dm->miss : nullptr, dm->capacity};
  dm->slots = fresh.slots;
  dm->source = fresh.source;
  if (fresh.miss) dm->miss = fresh.miss;
  dm->capacity = fresh.capacity;
  return old;
}

int lsa::dense::make_room(lsa_dense_map* dm, long long n, const char* who)
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
  TableArrays fresh{};
  if (const int rc = fresh_table(dm, cap, &fresh, who, "nothing was inserted")) return rc;
  if (dm->slots) dm->rehashes++;
  rehash_into(dm, fresh, Keep{nullptr, 0u, -1.});  // every voxel
  return LSA_OK;
}

int lsa::dense::room(lsa_dense_map* dm, std::initializer_list<Buffer> group, size_t* cap, size_t count, size_t slack, const char* who, const char* what,
                     const char* advice)
{
  lsa_ctx* ctx = dm->ctx;
  if (count <= *cap) return LSA_OK;
  *cap = 0;
  const size_t want = slack ? count + count / slack : count;
  size_t bytes = 0;
  for (const Buffer& b : group)
  {
    retire_dev(ctx, *b.at);
    *b.at = nullptr;
    bytes += want * b.elem;
  }
  for (const Buffer& b : group)
  {
    if (hipMalloc(b.at, want * b.elem) == hipSuccess) continue;
    (void)hipGetLastError();
    *b.at = nullptr;
    return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory for " + std::to_string(bytes) + " bytes of " + what + advice);
  }
  *cap = want;
  return LSA_OK;
}

FrameMove lsa::dense::frame_move(int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset)
{
  FrameMove m{};
  m.fused = 1;
  m.interpolate = interpolate ? 1 : 0;
  row_major_to_rt(H0, m.R.R, m.R.t);
  if (interpolate) m.c = make_interp_const(H0, H1, t0, t1);
  m.time_offset = time_offset;
  return m;
}

int lsa::dense::hold_frame(lsa_dense_map* dm)
{
  lsa_ctx* ctx = dm->ctx;
  LSA_HIP(ctx, hipEventRecord(dm->ev_frame, ctx->stream));
  LSA_HIP(ctx, hipStreamWaitEvent(dm->stream, dm->ev_frame, 0));
  return LSA_OK;
}

int lsa::dense::release_frame(lsa_dense_map* dm)
{
  lsa_ctx* ctx = dm->ctx;
  LSA_HIP(ctx, hipEventRecord(ctx->ev_dense, dm->stream));
  ctx->dense_frame_pending = true;
  return LSA_OK;
}

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
  // every device buffer of the map: the table, the words, and what scratch_room and room have grown
  void* const owned[] = {dm->slots,     dm->source,  dm->miss,    dm->stat,    dm->totals,         dm->slot_of,     dm->staged,       dm->staged_origins,
                         dm->chunks,    dm->keys[0], dm->keys[1], dm->index[0], dm->index[1],      dm->sort_tmp,    dm->out_pts,      dm->out_vox,
                         dm->out_src,   dm->out_miss, dm->viewpoints, dm->out_normals, dm->normal_sums, dm->grid_scratch, dm->grid_box, dm->cast_scratch};
  for (void* p : owned)
    if (p) (void)hipFree(p);
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
    // the bound of every ray's walk: ray_max_steps
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
  if (n == "CastSeconds") return dm->cast_seconds;
  if (n == "Rays" || n == "CastRays")
  {
    // the device's word, behind the calls in flight: the rays carved, and -- a word of their own -- the rays of
    // lsa_dense_map_cast and _compare_*, both since the last clear
    u64 rays = 0;
    if (settle(dm, "lsa_dense_map_get_param") != LSA_OK) return -1.;
    if (hipMemcpy(&rays, dm->stat + (n == "Rays" ? kStatRays : kStatCastRays), sizeof(u64), hipMemcpyDeviceToHost) != hipSuccess) return -1.;
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
  // the frame is whatever the context's stream has made of it so far (upload, times from the advancement)
  if (const int rc = hold_frame(dm)) return rc;
  // (a refusal comes from make_room, before anything is touched)
  const int rc = insert_device_points(dm, ctx->frame, ctx->frame_n, frame_move(interpolate, H0, H1, t0, t1, time_offset), frame, "lsa_dense_map_insert_frame");
  return rc ? rc : release_frame(dm);
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
  const int kept = compact_kept(dm, min_frames, max_miss_ratio, who);
  if (kept < 0) return kept;
  if (kept == occupied) return LSA_OK;  // nothing to remove: the table stays
  unsigned cap = kMinCapacity;
  while ((long long)(cap / 2) < (long long)kept) cap *= 2;  // kept <= occupied <= capacity / 2: never above the table's own
  TableArrays fresh{};
  rc = fresh_table(dm, cap, &fresh, who, "the map is as it was");
  if (rc) return rc;
  rehash_into(dm, fresh, keep_of(dm, min_frames, max_miss_ratio));  // (the predicate reads the old miss array)
  const unsigned serial = dm->next_serial++;
  hipLaunchKernelGGL(k_dense_publish, dim3(1), dim3(64), 0, dm->stream, dm->stat, dm->host_words, serial, (unsigned)kept);
  LSA_HIP(ctx, hipGetLastError());
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  adopt_published(dm, serial);  // the count the host took and k_dense_publish gave back
  *removed = occupied - kept;
  dm->pruned += *removed;
  return probe_ran_out(dm, who);
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

}  // extern "C"
