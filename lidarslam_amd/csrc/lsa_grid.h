// lsa_grid.h -- what the units of the device map share (internal): the state words and views the kernels work on, struct
// lsa_device_grid, and the host functions the units call in one another.  The head of lsa_device_grid.hip describes the
// data structure and says which job lives in which unit; lsa_device_grid_io.h is the narrow view other units get.
#pragma once
#include <algorithm>
#include <string>
#include "lsa_ctx.h"
#include "lsa_compact.h"
#include "lsa_wave.h"
#include "host/lsa_map_order.h"

namespace lsa
{
struct GridParams
{
  int grid_size;
  float resolution;   // (float)VoxelResolution
  double resolution_d;
  float leaf;         // (float)LeafSize
  double leaf_d;
  int sampling;
  unsigned min_frames;
};
// state the kernels read and write (device memory, kStInts ints)
enum { kStN = 0, kStNbPoints = 1, kStUpdated = 2, kStPosX = 3, kStGroups = 6, kStNew = 7, kStOff = 8, kStSub = 11, kStTmp = 12 /* 6 ints */, kStSubFirst = 18, kStCompact = 19, kStPred = 20 /* 6 ints: lo[3], hi[3]: outer voxels of the box a sub-map was extracted ahead for */,
       kStRec = 26 /* keys ClearOldPoints erased ("Ordered" = 0) */, kStInts = 32 };
__device__ __forceinline__ int round_to_int(float v)
{
  // Eigen's .round().cast<int>(): round half away from zero, then a C cast (out of range: INT_MIN, as on x86-64)
  const float r = roundf(v);
  return (r >= -2147483648.f && r < 2147483648.f) ? (int)r : (int)0x80000000;
}

struct MapView
{
  u64* keys;
  float4* pts;      // two float4 per voxel point
  unsigned* count;
};

// (the box in st[kStTmp .. +5] and lsa_device_grid_roll's box from the host: floats in the signed coding, f2os / os2f of lsa_wave.h)
__device__ __forceinline__ int lower_bound_u64(const u64* __restrict__ a, int n, u64 key)
{
  int lo = 0, hi = n;
  while (lo < hi)
  {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
}  // namespace lsa

struct lsa_device_grid
{
  lsa_ctx* ctx = nullptr;
  // parameters (RollingGrid.h:170-212)
  int GridSize = 50;
  double VoxelResolution = 10.;
  double LeafSize = 0.2;
  unsigned MinFramesPerVoxel = 0;
  int Sampling = 2;  // MAX_INTENSITY
  double DecayingThreshold = -1.;
  // the map
  lsa::MapView buf[2] = {};
  int cur = 0;
  int cap = 0;
  int n_upper = 0;  // upper bound of the number of voxels (what has been added so far)
  unsigned long long version = 0;  // modifications enqueued so far (Add, Roll, decay, Clear, Reset): what a reader of the map keeps its results by
  int* st = nullptr;           // device state (16 ints)
  int* host_st = nullptr;      // pinned copy of it, refreshed behind every modification
  hipEvent_t ev_state = nullptr;
  // The grid's kernels run on a stream beside the context's (by default the context's look-ahead stream, see
  // lsa_device_grid_create): a keyframe goes into the map beside the next frame's work on the context's stream (and may
  // be enqueued by another host thread).  Where the two meet -- keypoints read, a target or
  // the scratch buffer written -- events order them: ev_in (context -> grid) before, ev_out (grid -> context) after.
  hipStream_t stream = nullptr;
  bool own_stream = false, shared_stream = false;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_sub = nullptr, ev_ahead = nullptr;
  lsa::u64* host_sub = nullptr;     // coherent host memory: {tag, size} of the sub-map being built, one 8-byte store by the kernel
  unsigned sub_tag = 0;
  int sub_target = -1;         // target index (slot * 3 + type) of the sub-map between _begin and _end
  bool sub_pending = false;    // kernels of a sub-map are on their way
  // a sub-map extracted AHEAD of time for a predicted box, into the context's spare map target (target[9 + type])
  lsa::u64* host_ahead = nullptr;   // coherent host memory: [0] {tag, size} of the extraction, [1] {tag, same box?} of the check
  unsigned ahead_tag = 0;
  int ahead_phase = 0;         // 0 none, 1 extraction on its way, 2 search grid on its way / ready
  int ahead_type = -1, ahead_min = 0, ahead_m = 0;
  bool take_pending = false;   // a comparison of _take_begin is on its way
  int take_slot = 0;
  int staged = 0;              // keypoints staged in `batch` by lsa_device_grid_stage_keypoints
  bool submap_valid = false;
  int submap_count = 0;
  // batch scratch
  int bcap = 0;
  float4* batch = nullptr;
  lsa::u64 *bkeys = nullptr, *skeys = nullptr;
  unsigned *border = nullptr, *sorder = nullptr;
  int *heads = nullptr, *fresh_flag = nullptr, *chunks = nullptr;
  int* vrank = nullptr;  // CENTROID sampling: how many points of the batch that take part in the loop body lie in front of every point (arrival order), [n] = all
  int* old_local = nullptr;    // [cap] rank of an old voxel among the survivors of its chunk (Add)
  lsa::MapView fresh = {};
  int chunk_cap = 0;
  // the form of an insertion that keeps its scans in global memory (lsa_grid_add.hip): the exclusive scans of `chunks`
  // ([old chunks + 1]) and of `heads` ([blocks of the batch + 1]), and the block sums of every level of a scan
  int *oscan = nullptr, *fscan = nullptr, *scan_sums = nullptr;
  int oscan_cap = 0, fscan_cap = 0, scan_sums_cap = 0;
  int GlobalScans = 0;  // test knob: 0 by size, 1 that form at any size, 2 with scan blocks of 64 entries (levels end 16 times sooner)
  // "Ordered" = 0, the reference's container order (see the head of lsa_device_grid.hip)
  bool Ordered = true;
  lsa::host::KeyShadow shadow;  // keys-only copy of the reference's containers
  int rec_kind = 0;             // the record of the last modification on its way to the host: 0 none, kRecAdd, kRecRoll, kRecDecay
  int rec_grid = 0;             // the grid size it was made under
  int rec_voxels = 0;           // voxels of the map after the last record replayed: the shadow must hold as many
  hipEvent_t ev_rec = nullptr;  // behind its copy
  int* rec_st = nullptr;        // pinned: the state behind the modification (offset of the move, voxels created, keys erased)
  lsa::u64* rec_host = nullptr;      // pinned: the keys
  lsa::u64* rec_dev = nullptr;
  size_t rec_cap = 0;           // u64 of both
  bool order_stale = false;     // the shadow changed since the last upload
  int order_n = 0, order_cap = 0;
  lsa::u64* order_host = nullptr;    // pinned: the keys in the shadow's iteration order
  lsa::u64* order_dev = nullptr;
  int* perm = nullptr;          // [order_n]: place in the sorted array of the voxel at each rank of that order
  hipEvent_t ev_order = nullptr;
};

namespace lsa
{
#define G_HIP(call)                                                                                    \
  do                                                                                                   \
  {                                                                                                    \
    hipError_t e__ = (call);                                                                           \
    if (e__ != hipSuccess) return g->ctx->fail(LSA_E_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

// ---- lsa_device_grid.hip ----
void tighten(lsa_device_grid* g);
int after_submap(lsa_device_grid* g);
int order_after_context(lsa_device_grid* g);
GridParams params_of(const lsa_device_grid* g);
int alloc_view(lsa_device_grid* g, MapView& v, int cap);
void retire_view(lsa_device_grid* g, MapView& v);
int ensure_map(lsa_device_grid* g, int want);
int refresh_state(lsa_device_grid* g);
int begin_modification(lsa_device_grid* g, int voxels_wanted, size_t record_entries);
int end_modification(lsa_device_grid* g, int record_kind, size_t entries);
// ---- lsa_grid_add.hip ----
int ensure_batch(lsa_device_grid* g, int n);
int add_batches(lsa_device_grid* const* gs, const int* ns, int count, bool fixed, double time, bool do_roll);
// what one insertion addresses with an int: the voxels of the map and the points of the batch together (the kernels round both up
// to whole runs of the sort)
constexpr long long kAddressable = 0x7fffffffLL - 2 * 4096;
// ---- lsa_grid_order.hip ----
enum { kRecAdd = 1, kRecRoll = 2, kRecDecay = 3 };
int apply_record(lsa_device_grid* g);
int forget_records(lsa_device_grid* g);
int ensure_rec(lsa_device_grid* g, size_t entries);
int send_record(lsa_device_grid* g, int kind, size_t entries);
int ensure_order(lsa_device_grid* g);

// stable compaction of [0, n) on the map's stream (or `on`) with the map's chunk counts: lsa_compact.h
template <typename Pred, typename Emit>
void compact(lsa_device_grid* g, Pred pred, Emit emit, const int* n_ptr, int n_bound, int* total, bool append = false, bool copy_back = true,
             hipStream_t on = nullptr, u64* host_out = nullptr, unsigned host_tag = 0, int* clear_flag = nullptr)
{
  stable_compact(on ? on : g->stream, g->chunks, g->st + kStCompact, pred, emit, n_ptr, n_bound, total, append, copy_back, host_out, host_tag, clear_flag);
}
}  // namespace lsa
