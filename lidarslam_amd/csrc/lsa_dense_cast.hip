// lsa_dense_cast.hip -- rays through the dense map that stop at the first voxel that counts and report it (DESIGN.md 3.14
// "Rays"; the host statement, held byte for byte, is DenseMapHost.cast / .compare in lidarslam_amd/_dense_map.py).
//
// The walk is the carve's: dense_ray_begin / _next / _step of lsa_dense_table.h, with len + extend in place of len - margin.
// Every look-up is the read-only find(); nothing is claimed or written in the table, no thread waits for another, and a
// thread makes at most 3 * (max_range / leaf + 2) <= 3 * (4096 + 2) steps.  The calls first wait for the insertions and
// carves in flight (settle), so the slots read -- frames, first_frame, the miss word, the point, the source -- are final.
//   k_dense_cast     one thread a ray: walks until a voxel passes the predicate (the export's Keep, and first_frame < before
//                    under use_before), writes the 32-byte hit record and, when asked, the voxel's LidarPoint
//   k_dense_compare  the same walk from a frame point's origin to the point and `tolerance` past it; one label byte a point;
//                    the four counts take one atomic a wavefront and label (the ballot idiom of the carve's ray count).
//                    Unfused: world points and origins given.  Fused: the context's frame, point and origin made exactly as
//                    k_dense_carve makes them -- frame_point_to_world of the point and of the frame's own (0, 0, 0) at its time
// Lanes that hit early idle until the longest ray of their wavefront ends; that is accepted (a frame's neighbouring points
// have neighbouring rays).  The walk's state is the carve's (three axes of index, steps left, direction, tmax, tdelta, all in
// registers: the run-time axis of a step is written out, never an index into a private array) and two doubles more.
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "lsa_dense_table.h"

using namespace lsa;
using namespace lsa::dense;

namespace
{
struct Cast
{
  const float* origins;  // [n_origins][3] world positions (unfused compare, cast)
  int n_origins;         // 1 or n
  int n;
  double leaf, extend, range;
  long long max_steps;  // ray_max_steps
  Keep keep;            // frames >= min_frames, misses <= ratio * frames
  int use_before, before;
};

struct Hit  // lsa_dense_hit_t
{
  u64 key;
  float entry, exit, depth;
  int steps, source, status;
};
static_assert(sizeof(Hit) == 32 && sizeof(lsa_dense_hit_t) == 32, "a hit is one 32-byte record");

struct Walked
{
  int slot;   // of the hit, -1 for a miss
  int steps;  // voxels visited
  double t_in, t_out;
};

// from the ray's start voxel to the first that counts, or through the whole walk
__device__ __forceinline__ Walked walk_to_hit(const Cast& c, const Table& t, Ray& ray)
{
  Walked w{-1, 0, 0., 0.};
  double t_in = 0.;
  for (long long k = 0;; ++k)
  {
    double best;
    const int ax = dense_ray_next(ray, best);  // best: where the ray leaves this voxel
    const int s = t.slots ? find(t, dense_ray_key(ray)) : -1;
    if (s >= 0)
    {
      const Slot& S = t.slots[s];
      if (c.keep(S, (unsigned)s) && (!c.use_before || S.first < c.before))
      {
        w.slot = s;
        w.steps = (int)(k + 1);
        w.t_in = t_in;
        w.t_out = ax < 0 ? 1. : best;
        return w;
      }
    }
    if (k >= ray.total || ax < 0)
    {
      w.steps = (int)(k + 1);
      return w;
    }
    dense_ray_step(ray, ax);
    t_in = best;
  }
}

__global__ __launch_bounds__(256) void k_dense_cast(const float* __restrict__ targets, const Cast c, Table t, u64* __restrict__ stat, Hit* __restrict__ hits,
                                                    float4* __restrict__ points)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (r < c.n)
  {
    const float* of = c.origins + (c.n_origins == 1 ? (size_t)0 : 3 * (size_t)r);
    const float* tf = targets + 3 * (size_t)r;
    const double o[3] = {(double)of[0], (double)of[1], (double)of[2]};
    const double p[3] = {(double)tf[0], (double)tf[1], (double)tf[2]};
    Ray ray;
    ok = dense_ray_begin(o, p, c.extend, c.range, c.leaf, c.max_steps, ray);
    Hit h{0ull, 0.f, 0.f, 0.f, 0, 0, -1};
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (ok)
    {
      const Walked w = walk_to_hit(c, t, ray);
      h.steps = w.steps;
      h.status = 0;
      if (w.slot >= 0)
      {
        const Slot& S = t.slots[w.slot];
        a = S.a;
        b = S.b;
        h.key = S.key & ~kOccupied;
        h.entry = (float)(w.t_in * ray.tt);
        h.exit = (float)(w.t_out * ray.tt);
        const double d[3] = {p[0] - o[0], p[1] - o[1], p[2] - o[2]};
        h.depth = (float)(((((double)a.x - o[0]) * d[0] + ((double)a.y - o[1]) * d[1]) + ((double)a.z - o[2]) * d[2]) / ray.len);
        h.source = t.source[w.slot];
        h.status = 1;
      }
    }
    hits[r] = h;
    if (points)
    {
      points[2 * (size_t)r] = a;
      points[2 * (size_t)r + 1] = b;
    }
  }
  add_once_a_wavefront(&stat[kStatCastRays], ok);
}

__global__ __launch_bounds__(256) void k_dense_compare(const float4* __restrict__ in, const FrameMove m, const Cast c, Table t, u64* __restrict__ stat,
                                                       unsigned char* __restrict__ labels)
{
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  int label = -1;
  if (r < c.n)
  {
    float4 a = in[2 * (size_t)r];
    float4 b = in[2 * (size_t)r + 1];
    float ofx, ofy, ofz;
    if (m.fused)
    {
      // as k_dense_carve: the sensor at the time the point was measured, and the point, in the world
      float4 oa = make_float4(0.f, 0.f, 0.f, a.w), ob = b;
      frame_point_to_world(oa, ob, m.interpolate, m.c, m.R, m.time_offset);
      frame_point_to_world(a, b, m.interpolate, m.c, m.R, m.time_offset);
      ofx = oa.x; ofy = oa.y; ofz = oa.z;
    }
    else
    {
      const float* of = c.origins + (c.n_origins == 1 ? (size_t)0 : 3 * (size_t)r);
      ofx = of[0]; ofy = of[1]; ofz = of[2];
    }
    const double o[3] = {(double)ofx, (double)ofy, (double)ofz};
    const double p[3] = {(double)a.x, (double)a.y, (double)a.z};
    Ray ray;
    ok = dense_ray_begin(o, p, c.extend, c.range, c.leaf, c.max_steps, ray);
    label = 0;  // NOT_JUDGED: no ray, or a point beyond the range
    if (ok && !(ray.len > c.range))
    {
      const Walked w = walk_to_hit(c, t, ray);
      // decided in double: the ray left a voxel that counts more than the tolerance before the point
      label = w.slot < 0 ? 2 : (w.t_out * ray.tt < ray.len - c.extend ? 3 : 1);
    }
    labels[r] = (unsigned char)label;
  }
  add_once_a_wavefront(&stat[kStatCastRays], ok);
#pragma unroll
  for (int l = 0; l < 4; ++l) add_once_a_wavefront(&stat[kStatLabels + l], label == l);
}

// LSA_E_ARG for what the statement refuses; nothing has been touched
int check_params(lsa_dense_map* dm, const lsa_dense_cast_params_t* p, bool compare, const char* who)
{
  lsa_ctx* ctx = dm->ctx;
  if (!p) return ctx->fail(LSA_E_ARG, std::string(who) + ": no parameters");
  if (!std::isfinite(p->max_range) || !(p->max_range > 0.) || !(p->max_range / dm->leaf <= kMaxRangeLeaves))
    return ctx->fail(LSA_E_ARG, std::string(who) + ": max_range finite, positive and at most 4096 leaves");
  if (std::isnan(p->extend)) return ctx->fail(LSA_E_ARG, std::string(who) + ": extend is NaN");
  if (compare && (!std::isfinite(p->extend) || p->extend < 0.)) return ctx->fail(LSA_E_ARG, std::string(who) + ": the tolerance (extend) finite and >= 0");
  if (std::isnan(p->max_miss_ratio)) return ctx->fail(LSA_E_ARG, std::string(who) + ": max_miss_ratio is NaN");
  if (p->min_frames < 1) return ctx->fail(LSA_E_ARG, std::string(who) + ": min_frames >= 1");
  if (p->use_before != 0 && p->use_before != 1) return ctx->fail(LSA_E_ARG, std::string(who) + ": use_before is 0 or 1");
  if (p->reserved != 0) return ctx->fail(LSA_E_ARG, std::string(who) + ": reserved is 0");
  return LSA_OK;
}

Cast cast_of(const lsa_dense_map* dm, const lsa_dense_cast_params_t* p, int n, const float* origins, int n_origins)
{
  Cast c{};
  c.origins = origins;
  c.n_origins = n_origins;
  c.n = n;
  c.leaf = dm->leaf;
  c.extend = p->extend;
  c.range = p->max_range;
  c.max_steps = ray_max_steps(p->max_range, dm->leaf);
  c.keep = keep_of(dm, p->min_frames, p->max_miss_ratio);  // (min_frames >= 1: check_params)
  c.use_before = p->use_before;
  c.before = p->before;
  return c;
}

// `bytes` of device scratch for one call; LSA_E_CAPACITY without memory
int cast_room(lsa_dense_map* dm, size_t bytes, const char* who)
{
  return room(dm, {{(void**)&dm->cast_scratch, 1}}, &dm->cast_scratch_cap, bytes, 2, who, "rays", "; ask for fewer in one call");
}

constexpr size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// the launch over n points at `src` (device) and the download of labels and counts; the map is settled.  A fused call reads the
// context's frame: the event its next writer waits for is recorded behind the launch, which reads the buffer last
int compare_device_points(lsa_dense_map* dm, const lsa_point_t* src, int n, const FrameMove& m, const Cast& c, unsigned char* labels_dev, uint8_t* labels,
                          long long counts[4])
{
  lsa_ctx* ctx = dm->ctx;
  LSA_HIP(ctx, hipMemsetAsync(dm->stat + kStatLabels, 0, 4 * sizeof(u64), dm->stream));
  {
    // per point 32 B (unfused: and 12 B of origin) read, 1 B written; per visited voxel an 8-byte key at least -- not known here
    ProfScope ps(ctx, "dense_compare", (double)n * (m.fused ? 33 : 45), dm->stream);
    hipLaunchKernelGGL(k_dense_compare, dim3((n + 255) / 256), dim3(256), 0, dm->stream, reinterpret_cast<const float4*>(src), m, c, table_of(dm), dm->stat,
                       labels_dev);
  }
  LSA_HIP(ctx, hipGetLastError());
  if (m.fused)
  {
    if (const int rc = release_frame(dm)) return rc;
  }
  u64 words[4] = {0, 0, 0, 0};
  std::vector<uint8_t> got((size_t)n);  // the caller's labels stay untouched unless everything arrives
  LSA_HIP(ctx, hipMemcpyAsync(got.data(), labels_dev, (size_t)n, hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipMemcpyAsync(words, dm->stat + kStatLabels, sizeof(words), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  std::memcpy(labels, got.data(), (size_t)n);
  for (int l = 0; l < 4; ++l) counts[l] = (long long)words[l];
  return LSA_OK;
}
}  // namespace

extern "C" {

int lsa_dense_map_cast(lsa_dense_map* dm, const float* origins_xyz, int n_origins, const float* targets_xyz, int n, const lsa_dense_cast_params_t* params,
                       lsa_dense_hit_t* hits, lsa_point_t* points)
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_cast";
  if (n < 0 || !origins_xyz || !targets_xyz || !hits || (n_origins != 1 && n_origins != n)) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument (one origin, or one per ray)");
  if (const int rc = check_params(dm, params, false, who)) return rc;
  if (n == 0) return LSA_OK;
  const double started = now_seconds();
  int rc = settle(dm, who);
  if (rc) return rc;
  const size_t origins_bytes = up16((size_t)n_origins * 12), targets_bytes = up16((size_t)n * 12), hits_bytes = (size_t)n * sizeof(Hit);
  rc = cast_room(dm, origins_bytes + targets_bytes + hits_bytes + (points ? (size_t)n * sizeof(lsa_point_t) : 0), who);
  if (rc) return rc;
  float* origins_dev = reinterpret_cast<float*>(dm->cast_scratch);
  float* targets_dev = reinterpret_cast<float*>(dm->cast_scratch + origins_bytes);
  Hit* hits_dev = reinterpret_cast<Hit*>(dm->cast_scratch + origins_bytes + targets_bytes);
  float4* points_dev = points ? reinterpret_cast<float4*>(dm->cast_scratch + origins_bytes + targets_bytes + hits_bytes) : nullptr;
  LSA_HIP(ctx, hipMemcpyAsync(origins_dev, origins_xyz, (size_t)n_origins * 12, hipMemcpyHostToDevice, dm->stream));
  LSA_HIP(ctx, hipMemcpyAsync(targets_dev, targets_xyz, (size_t)n * 12, hipMemcpyHostToDevice, dm->stream));
  {
    // per ray 24 B read and 32 (64) B written; per visited voxel an 8-byte key at least -- not known here
    ProfScope ps(ctx, "dense_cast", (double)n * (points ? 88 : 56), dm->stream);
    hipLaunchKernelGGL(k_dense_cast, dim3((n + 255) / 256), dim3(256), 0, dm->stream, targets_dev, cast_of(dm, params, n, origins_dev, n_origins), table_of(dm), dm->stat,
                       hits_dev, points_dev);
  }
  LSA_HIP(ctx, hipGetLastError());
  LSA_HIP(ctx, hipMemcpyAsync(hits, hits_dev, hits_bytes, hipMemcpyDeviceToHost, dm->stream));
  if (points) LSA_HIP(ctx, hipMemcpyAsync(points, points_dev, (size_t)n * sizeof(lsa_point_t), hipMemcpyDeviceToHost, dm->stream));
  LSA_HIP(ctx, hipStreamSynchronize(dm->stream));
  dm->cast_seconds = now_seconds() - started;
  return LSA_OK;
}

int lsa_dense_map_compare_points(lsa_dense_map* dm, const lsa_point_t* pts, int n, const float* origins_xyz, int n_origins, const lsa_dense_cast_params_t* params,
                                 uint8_t* labels, long long counts[4])
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_compare_points";
  if (n < 0 || !pts || !origins_xyz || !labels || !counts || (n_origins != 1 && n_origins != n))
    return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument (one origin, or one per point)");
  if (const int rc = check_params(dm, params, true, who)) return rc;
  if (n == 0)
  {
    for (int l = 0; l < 4; ++l) counts[l] = 0;
    return LSA_OK;
  }
  const double started = now_seconds();
  int rc = settle(dm, who);
  if (rc) return rc;
  const size_t points_bytes = (size_t)n * sizeof(lsa_point_t), origins_bytes = up16((size_t)n_origins * 12);
  rc = cast_room(dm, points_bytes + origins_bytes + (size_t)n, who);
  if (rc) return rc;
  lsa_point_t* points_dev = reinterpret_cast<lsa_point_t*>(dm->cast_scratch);
  float* origins_dev = reinterpret_cast<float*>(dm->cast_scratch + points_bytes);
  unsigned char* labels_dev = dm->cast_scratch + points_bytes + origins_bytes;
  LSA_HIP(ctx, hipMemcpyAsync(points_dev, pts, points_bytes, hipMemcpyHostToDevice, dm->stream));
  LSA_HIP(ctx, hipMemcpyAsync(origins_dev, origins_xyz, (size_t)n_origins * 12, hipMemcpyHostToDevice, dm->stream));
  FrameMove m{};
  rc = compare_device_points(dm, points_dev, n, m, cast_of(dm, params, n, origins_dev, n_origins), labels_dev, labels, counts);
  dm->cast_seconds = now_seconds() - started;
  return rc;
}

int lsa_dense_map_compare_frame(lsa_dense_map* dm, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset,
                                const lsa_dense_cast_params_t* params, uint8_t* labels, int capacity, long long counts[4])
{
  if (!dm) return LSA_E_ARG;
  lsa_ctx* ctx = dm->ctx;
  const char* who = "lsa_dense_map_compare_frame";
  if (!H0 || (interpolate && !H1) || !labels || !counts || capacity < 0) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  if (const int rc = check_params(dm, params, true, who)) return rc;
  if (!ctx->frame || ctx->frame_n <= 0) return ctx->fail(LSA_E_STATE, std::string(who) + ": no frame");
  const int n = ctx->frame_n;
  if (n > capacity) return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": the frame has " + std::to_string(n) + " points, the labels have room for " + std::to_string(capacity));
  const double started = now_seconds();
  int rc = settle(dm, who);
  if (rc) return rc;
  rc = cast_room(dm, (size_t)n, who);
  if (rc) return rc;
  // as the fused carve
  rc = hold_frame(dm);
  if (rc) return rc;
  rc = compare_device_points(dm, ctx->frame, n, frame_move(interpolate, H0, H1, t0, t1, time_offset), cast_of(dm, params, n, nullptr, 0), dm->cast_scratch, labels, counts);
  if (rc) return rc;
  dm->cast_seconds = now_seconds() - started;
  return n;
}

int lsa_scan_targets(const double pose16[16], const double* elevations_rad, int n_rings, int n_azimuth, float* origin_xyz, float* targets_xyz)
{
  if (!pose16 || !elevations_rad || !origin_xyz || !targets_xyz || n_rings < 0 || n_azimuth < 0) return LSA_E_ARG;
  for (int k = 0; k < 3; ++k) origin_xyz[k] = (float)pose16[4 * k + 3];
  const double two_pi = 6.283185307179586476925286766559;
  for (int r = 0; r < n_rings; ++r)
  {
    const double ce = std::cos(elevations_rad[r]), se = std::sin(elevations_rad[r]);
    for (int c = 0; c < n_azimuth; ++c)
    {
      const double az = two_pi * (double)c / (double)n_azimuth;
      const double v[3] = {ce * std::cos(az), ce * std::sin(az), se};
      float* out = targets_xyz + 3 * ((size_t)r * (size_t)n_azimuth + (size_t)c);
      for (int k = 0; k < 3; ++k) out[k] = (float)(((pose16[4 * k] * v[0] + pose16[4 * k + 1] * v[1]) + pose16[4 * k + 2] * v[2]) + pose16[4 * k + 3]);
    }
  }
  return LSA_OK;
}

}  // extern "C"
