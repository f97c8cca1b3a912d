// lsa_dense_carve.hip -- free space in the dense map (DESIGN.md 3.14 "Free space"; the host statement, held byte for byte, is
// DenseMapHost.carve in lidarslam_amd/_dense_map.py).
//
// miss[2 * capacity], made by the first carve -- a map never carved has none and pays for none --: the voxel's misses, then
// the word of the last ordinal that counted one (last_word: the zeroed word is "none").
//   k_dense_carve   one thread per ray walks the voxels from the sensor to shortly before the point -- a number of steps
//                   known before the first -- and looks each up without ever claiming; a voxel found whose last_frame is
//                   not the ordinal takes atomicMax on its word, and the one thread that raised it adds the miss
// It runs behind k_dense_apply of its ordinal on the same stream, so last_frame is final.  The array is carried by the rehash
// (lsa_dense_map.hip), merged by the re-projection (atomicAdd, atomicMax), read by the export's predicate.
#include <cmath>
#include "lsa_dense_table.h"

using namespace lsa;
using namespace lsa::dense;

namespace
{
struct Carve
{
  const float* origins;  // unfused: [n_origins][3] world positions of the sensor
  int n_origins;         // 1 or the number of points
  int stride;            // ray r belongs to point r * stride
  int rays;
  int frame;
  double leaf, margin, range;  // margin = margin_leaves * leaf
  long long max_steps;         // ray_max_steps
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
  add_once_a_wavefront(&stat[kStatRays], ok);
  if (!ok) return;
  const unsigned word = last_word(c.frame);
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
    // as a fresh table's: an array whose zeroing was refused is not kept
    const size_t bytes = (size_t)dm->capacity * 2 * sizeof(unsigned);
    hipError_t e = hipSuccess;
    dm->miss = static_cast<unsigned*>(fresh_zeroed(dm, bytes, &e));
    if (e == hipErrorOutOfMemory) return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": no device memory for " + std::to_string(bytes) + " bytes of misses; nothing was carved");
    if (e != hipSuccess) return ctx->fail(LSA_E_HIP, std::string(who) + ": hipMemsetAsync: " + hipGetErrorString(e));
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
  c.max_steps = ray_max_steps(dm->carve_range, dm->leaf);
  {
    // per ray 32 B (and 12 B of origin) read; per visited voxel an 8-byte key at least -- not known here
    ProfScope ps(ctx, "dense_carve", (double)c.rays * 44, dm->stream);
    hipLaunchKernelGGL(k_dense_carve, dim3((c.rays + 255) / 256), dim3(256), 0, dm->stream, reinterpret_cast<const float4*>(src), m, c, table_of(dm), dm->stat);
  }
  dm->last_frame = frame;
  return LSA_OK;
}
}  // namespace

extern "C" {

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
  // as the fused insertion; the carve reads the buffer last
  if (const int rc = hold_frame(dm)) return rc;
  if (const int rc = carve_device_points(dm, ctx->frame, ctx->frame_n, frame_move(interpolate, H0, H1, t0, t1, time_offset), nullptr, 0, frame, who)) return rc;
  if (const int rc = release_frame(dm)) return rc;
  dm->carve_seconds = now_seconds() - started;
  return LSA_OK;
}

}  // extern "C"
