// lsa_dense_reproject.hip -- the dense map under a corrected trajectory (DESIGN.md 3.14 "Re-projection"; the host statement,
// held byte for byte, is DenseMapHost.reproject in lidarslam_amd/_dense_map.py).  Not on the frame path.
//
// source[capacity] is what lets a corrected trajectory move the map: every voxel's point under the correction of the frame
// that measured it, re-keyed into a fresh table of the same capacity, voxels that meet merged -- three launches, one thread
// per old slot, under the same rules as the insertion:
//   k_dense_move    moves the point, finds or claims its slot in the new table, adds count and frames, folds first / last
//                   and the candidate word (intensity code << 32) | ~ordered(source) in with atomics, notes the new slot
//   k_dense_elect   the old slots whose word the candidate names atomicMin their old key: ties on intensity and source
//   k_dense_settle  the old slot named by both writes the moved point and its source, caps frames, disarms the word
// The miss array of a map that has been carved is merged with atomicAdd and atomicMax.
#include "lsa_dense_table.h"
#include "lsa_device_math.h"

using namespace lsa;
using namespace lsa::dense;

namespace
{
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

// first_frame / last_frame of a slot of the new table are folded as first_word / last_word; k_dense_settle decodes them.
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
// publishes the counts as k_dense_apply does, and the voxels dropped
__global__ __launch_bounds__(256) void k_dense_settle(const Reproject r, Table t, const u64* __restrict__ stat, u64* __restrict__ host_words, unsigned serial)
{
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) publish_counts(stat, host_words, serial, true);
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
  const int first = first_of_word(__builtin_bit_cast(unsigned, S.first)), last = last_of_word(__builtin_bit_cast(unsigned, S.last));
  S.first = first;
  S.last = last;
  const u64 span = (u64)((long long)last - (long long)first + 1ll), sum = r.frames[s];
  S.frames = (unsigned)(sum < span ? sum : span);
  S.cand = 0ull;
}
}  // namespace

extern "C" int lsa_dense_map_reproject(lsa_dense_map* dm, const double* corrections16, int first_frame, int n, long long* dropped)
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
  TableArrays fresh{};
  rc = fresh_table(dm, cap, &fresh, who, "the map is as it was");
  if (rc)
  {
    (void)hipFree(corrections);
    (void)hipFree(scratch);
    return rc;
  }
  // from here on the old table belongs to the graveyard and the new one is the map's, whatever a launch answers
  const TableArrays old = swap_table(dm, fresh);
  Reproject r;
  r.old = old.slots;
  r.old_source = old.source;
  r.old_miss = old.miss;
  r.old_capacity = cap;
  r.corrections = corrections;
  r.first_frame = first_frame;
  r.n = n;
  r.leaf = dm->leaf;
  r.pick = reinterpret_cast<u64*>(scratch);
  r.frames = r.pick + cap;
  r.to = reinterpret_cast<int*>(r.frames + cap);
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
  retire_dev(ctx, old.slots);
  retire_dev(ctx, old.source);
  retire_dev(ctx, old.miss);
  retire_dev(ctx, corrections);
  retire_dev(ctx, scratch);
  if (e != hipSuccess) return ctx->fail(LSA_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
  adopt_published(dm, serial);  // the new table's count
  *dropped = (long long)__atomic_load_n(&dm->host_words[3], __ATOMIC_ACQUIRE);
  dm->dropped += *dropped;
  dm->reprojections++;
  dm->reproject_seconds = now_seconds() - t0;
  return probe_ran_out(dm, who);
}
