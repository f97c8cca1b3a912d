// lsa_dense_export.hip -- what the dense map hands out (DESIGN.md 3.14 "Export"; the host statement, held byte for byte, is
// DenseMapHost.export in lidarslam_amd/_dense_map.py).  Not on the frame path.
//
// lsa_compact.h's stable compaction of the slots that pass the predicate (Keep: min_frames, the miss ratio), rocprim's radix
// sort by key -- this is the only unit of the map that includes rocprim --, and a gather (k_dense_gather) of the points, the
// voxel records, the sources and the misses into columns kept on the device for the getters and the PCD writer.  The normals
// (lsa_dense_normals.hip) and the prune (lsa_dense_map.hip) start from the same compaction.
#include <rocprim/device/device_radix_sort.hpp>
#include <new>
#include "lsa_compact.h"
#include "lsa_dense_table.h"
#include "lsa_device_grid_io.h"
#include "host/lsa_pcd.h"

using namespace lsa;
using namespace lsa::dense;

namespace
{
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

// one 4-byte column of the export to the caller, the sources or the misses: lsa_dense_map_get_sources_filtered and _get_misses
int get_column(lsa_dense_map* dm, int min_frames, double max_miss_ratio, void* out, bool misses, int capacity, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  if (capacity < 0) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  const int kept = export_sorted(dm, min_frames, max_miss_ratio, who);
  if (kept <= 0) return kept;
  const int n = std::min(kept, capacity);
  const void* column = misses ? (const void*)dm->out_miss : (const void*)dm->out_src;  // (where this export left them)
  if (n > 0 && out) LSA_HIP(ctx, hipMemcpyAsync(out, column, (size_t)n * 4, hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  return kept;
}
}  // namespace

int lsa::dense::compact_kept(lsa_dense_map* dm, int min_frames, double max_miss_ratio, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  const int occupied = (int)occupied_bound(dm);  // exact: everything enqueued has been published
  if (occupied <= 0 || !dm->slots) return 0;
  const int nchunks = (int)((dm->capacity + 1023u) / 1024u);
  if (const int rc = scratch_room(ctx, &dm->chunks, (int**)nullptr, &dm->chunks_cap, (size_t)nchunks, 64)) return rc;
  if (const int rc = room(dm, {{(void**)&dm->keys[0], sizeof(u64)}, {(void**)&dm->index[0], sizeof(unsigned)}, {(void**)&dm->keys[1], sizeof(u64)},
                               {(void**)&dm->index[1], sizeof(unsigned)}}, &dm->keys_cap, (size_t)occupied, 2, who, "keys and slots"))
    return rc;
  const Slot* slots = dm->slots;
  stable_compact(dm->stream, dm->chunks, dm->totals + 1, ExportPred{slots, keep_of(dm, min_frames, max_miss_ratio)}, ExportEmit{slots, dm->keys[0], dm->index[0]},
                 (const int*)nullptr, (int)dm->capacity, dm->totals);
  int kept = 0;
  LSA_HIP(ctx, hipMemcpyAsync(&kept, dm->totals, sizeof(int), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  return std::max(kept, 0);
}

int lsa::dense::export_sorted(lsa_dense_map* dm, int min_frames, double max_miss_ratio, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  const int rc = settle(dm, who);
  if (rc) return rc;
  const int kept = compact_kept(dm, min_frames, max_miss_ratio, who);
  if (kept <= 0) return kept;
  size_t tmp_bytes = 0;
  LSA_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_bytes, dm->keys[0], dm->keys[1], dm->index[0], dm->index[1], (size_t)kept, 0u, 63u, dm->stream));
  if (const int rc = room(dm, {{(void**)&dm->sort_tmp, 1}}, &dm->sort_tmp_cap, tmp_bytes, 0, who, "sort scratch")) return rc;
  LSA_HIP(ctx, rocprim::radix_sort_pairs(dm->sort_tmp, tmp_bytes, dm->keys[0], dm->keys[1], dm->index[0], dm->index[1], (size_t)kept, 0u, 63u, dm->stream));
  if (const int rc = room(dm, {{(void**)&dm->out_pts, sizeof(lsa_point_t)}, {(void**)&dm->out_vox, sizeof(lsa_dense_voxel_t)}, {(void**)&dm->out_src, sizeof(int)},
                               {(void**)&dm->out_miss, sizeof(unsigned)}}, &dm->out_cap, (size_t)kept, 2, who, "export columns"))
    return rc;
  hipLaunchKernelGGL(k_dense_gather, dim3((kept + 255) / 256), dim3(256), 0, dm->stream, dm->slots, dm->source, dm->miss, dm->keys[1], dm->index[1], kept,
                     reinterpret_cast<float4*>(dm->out_pts), dm->out_vox, dm->out_src, dm->out_miss);
  return kept;
}

extern "C" {

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

int lsa_dense_map_get_sources_filtered(lsa_dense_map* dm, int min_frames, double max_miss_ratio, int* out, int capacity)
{
  if (!dm) return LSA_E_ARG;
  return get_column(dm, min_frames, max_miss_ratio, out, false, capacity, "lsa_dense_map_get_sources");
}

int lsa_dense_map_get_misses(lsa_dense_map* dm, int min_frames, double max_miss_ratio, uint32_t* out, int capacity)
{
  if (!dm) return LSA_E_ARG;
  return get_column(dm, min_frames, max_miss_ratio, out, true, capacity, "lsa_dense_map_get_misses");
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
    std::fill(ctx->pcd_times, ctx->pcd_times + 8, 0.);
    const double t0 = now_seconds();
    const int kept = export_sorted(dm, min_frames, max_miss_ratio, "lsa_dense_map_save_pcd");
    if (kept < 0) return kept;
    ctx->pcd_times[4] = now_seconds() - t0;
    return pcd_save_device_points(ctx, dm->stream, dm->out_pts, kept, path, format);
  }
  catch (const std::bad_alloc&) { return ctx->fail(LSA_E_CAPACITY, std::string(path) + ": not enough host memory"); }
}

}  // extern "C"
