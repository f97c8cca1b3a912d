// lsa_dense_normals.hip -- oriented surface normals per voxel of the dense map (DESIGN.md 3.14 "Normals"; the host statement,
// held byte for byte, is DenseMapHost.normals in lidarslam_amd/_dense_map.py).  Not on the frame path, nothing stored: behind
// the export's compaction and sort (lsa_dense_export.hip)
//   k_dense_normals         a group of 32 lanes a voxel probes the surrounding cells, packs the neighbours found into LDS in cell
//                           order and adds the nine sums up in that order
//   k_dense_normal_records  one thread a voxel: covariance, eigen33<double>, the sign towards the viewpoint, the record
#include <cstring>
#include <new>
#include <vector>
#include "lsa_dense_table.h"
#include "lsa_device_grid_io.h"
#include "lsa_device_math.h"
#include "host/lsa_pcd.h"

using namespace lsa;
using namespace lsa::dense;

namespace
{
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

// steps 4 to 7 of the definition: the record of a voxel from its count and sums
__device__ __forceinline__ void normal_record(const Normals& c, const Table& t, unsigned slot, const double p[3], unsigned k, const double s[3], const double S[6],
                                              unsigned* __restrict__ o)
{
  o[4] = k;
  o[0] = o[1] = o[2] = o[3] = kQuietNaN;
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
    ix = key_index(key, 0);
    iy = key_index(key, 1);
    iz = key_index(key, 2);
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
}  // namespace

extern "C" {

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
    std::fill(ctx->pcd_times, ctx->pcd_times + 8, 0.);
    const double t0 = now_seconds();
    const int kept = normals_sorted(dm, min_frames, max_miss_ratio, radius_leaves, min_neighbors, viewpoints_xyz, n_viewpoints, first_frame, who);
    if (kept <= 0) return kept;
    // the four floats of every record, for the writer to put behind the point (the path is not hot)
    std::vector<lsa_dense_normal_t> records((size_t)kept);
    LSA_HIP(ctx, hipMemcpyAsync(records.data(), dm->out_normals, (size_t)kept * sizeof(lsa_dense_normal_t), hipMemcpyDeviceToHost, dm->stream));
    LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
    std::vector<float> normals4((size_t)kept * 4);
    for (int i = 0; i < kept; ++i) std::memcpy(&normals4[(size_t)i * 4], &records[(size_t)i], 4 * sizeof(float));
    ctx->pcd_times[4] = now_seconds() - t0;
    return pcd_save_device_points(ctx, dm->stream, dm->out_pts, kept, path, format, normals4.data());
  }
  catch (const std::bad_alloc&) { return ctx->fail(LSA_E_CAPACITY, std::string(path) + ": not enough host memory"); }
}

}  // extern "C"
