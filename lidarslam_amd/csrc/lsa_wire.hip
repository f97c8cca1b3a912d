// lsa_wire.hip -- the sensors' own formats straight to the device as LidarPoints: Velodyne driver records, LidarView
// structures of arrays (polydata), RoboSense organized clouds.  The two that drop points do it with lsa_compact.h.
#include <cmath>
#include "lsa_ctx.h"
#include "lsa_compact.h"
#include "lsa_wave.h"
#include "../../include/lsa_pmath.h"

using namespace lsa;

extern "C" {

namespace
{
// one LidarPoint as the two float4 it is made of: time bits low / high, intensity, laser_id u16 | device_id u8 << 16, label u8 = 0
__device__ __forceinline__ void store_lidar_point(float4* __restrict__ out, size_t at, float x, float y, float z, double time, float intensity, unsigned laser_id,
                                                  int device_id)
{
  const long long tb = __double_as_longlong(time);
  float4 a = make_float4(x, y, z, 1.f);
  float4 b;
  b.x = __int_as_float((int)(tb & 0xffffffffll));
  b.y = __int_as_float((int)(tb >> 32));
  b.z = intensity;
  b.w = __uint_as_float(laser_id | ((unsigned)(device_id & 0xff) << 16));
  out[2 * at] = a;
  out[2 * at + 1] = b;
}
// LaserIdMapping when one is given (0xffff behind its end), `unmapped` otherwise
__host__ __device__ __forceinline__ unsigned mapped_laser_id(const uint16_t* mapping, int mapping_len, size_t raw, unsigned unmapped) { return mapping_len > 0 ? (raw < (size_t)mapping_len ? mapping[raw] : 0xffffu) : unmapped; }

// What the two uploads that drop points end with: frame_own holds the converted points, *total_dev how many.  The frame
// becomes the current one; on the first usable frame the azimuthal resolution is estimated on the host from the converted
// points (SSKE.cxx:593-637).  kept_out may be null.
int adopt_compacted_frame(lsa_ctx* ctx, const int* total_dev, int* kept_out)
{
  int kept = 0;
  LSA_HIP(ctx, hipMemcpyAsync(&kept, total_dev, sizeof(kept), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's arrays may go away; the size (and what else was read back) is needed now
  if (kept_out) *kept_out = kept;
  ctx->frame = kept > 0 ? ctx->frame_own : nullptr;
  ctx->frame_n = kept;
  ctx->inbox_current = -1;
  if (kept > 0 && (ctx->az_res < 1e-6 || M_PI / 4. < ctx->az_res))
  {
    std::vector<lsa_point_t> pts(kept);
    LSA_HIP(ctx, hipMemcpy(pts.data(), ctx->frame_own, (size_t)kept * sizeof(lsa_point_t), hipMemcpyDeviceToHost));
    maybe_estimate_resolution(ctx, pts.data(), kept);
  }
  return LSA_OK;
}

// ---- the driver's wire format straight to the device --------------------------------------
struct WireMap
{
  int advancement;  // 1: the time field receives the azimuth advancement in [0, 1) instead of the record's time
  lsa_wire_layout_t lay;
  int mapping_len;
  int device_id;
  uint16_t mapping[kMaxRings];
};
// one LidarPoint per wire record (VelodyneToLidarNode.cxx:81-96): coordinates, intensity, mapped ring, device,
// time offset widened to double
__global__ __launch_bounds__(256) void k_wire_to_points(const unsigned char* __restrict__ raw, int n, WireMap m, float4* __restrict__ out)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned char* r = raw + (size_t)i * m.lay.point_step;
  auto f32 = [&](int off) { float v; memcpy(&v, r + off, sizeof(v)); return v; };
  uint16_t ring;
  memcpy(&ring, r + m.lay.off_ring, sizeof(ring));
  const unsigned id = mapped_laser_id(m.mapping, m.mapping_len, ring, ring);
  double t = (double)f32(m.lay.off_time);
  if (m.advancement)
  {
    // SpinningFrameAdvancementEstimator (lidar_conversions/src/Utilities.h:88-100): the azimuth of the point as a
    // fraction of a turn, relative to the frame's first point, wrapped into [0, 1).  std::fmod is exact, and so is
    // x - trunc(x) for |x| < 2^52: wrap() below IS std::fmod(1 + std::fmod(x, 1), 1).  The arc tangent is the portable
    // one evaluated in double and rounded to float (the node calls the float overload).
    auto adv_of = [&](const unsigned char* rr) {
      float x, y;
      memcpy(&x, rr + m.lay.off_x, sizeof(x));
      memcpy(&y, rr + m.lay.off_y, sizeof(y));
      return (3.14159265358979323846 - (double)(float)lsa_atan2((double)y, (double)x)) / (2 * 3.14159265358979323846);
    };
    auto wrap = [](double x) { const double f = x - trunc(x); const double g = 1.0 + f; return g - trunc(g); };
    t = wrap(adv_of(r) - adv_of(raw));
  }
  store_lidar_point(out, i, f32(m.lay.off_x), f32(m.lay.off_y), f32(m.lay.off_z), t, f32(m.lay.off_intensity), id, m.device_id);
}
// lidar_conversions::Utils::SpinningFrameAdvancementEstimator (ros_wrapping/lidar_conversions/src/Utilities.h:62-114)
struct FrameAdvancementEstimator
{
  double init = 0.;
  bool first = true;
  std::vector<double> prev = std::vector<double>(65536, 0.);  // std::map<int, double>: a missing ring reads 0
  double operator()(float x, float y, unsigned laser_id)
  {
    const double adv = (M_PI - std::atan2(y, x)) / (2 * M_PI);
    if (first) { init = adv; first = false; }
    auto wrapMax = [](double v, double max) { return std::fmod(max + std::fmod(v, max), max); };
    double frameAdv = wrapMax(adv - init, 1.);
    if (frameAdv < prev[laser_id]) frameAdv += 1.;
    prev[laser_id] = frameAdv;
    return frameAdv;
  }
};
}  // namespace

int lsa_upload_wire_frame(lsa_ctx* ctx, const void* data, int n, const lsa_wire_layout_t* lay, const uint16_t* laser_id_mapping, int mapping_len,
                          int device_id, double rpm, int timestamp_first_packet)
{
  if (!ctx || !data || !lay || n <= 0 || lay->point_step <= 0 || mapping_len < 0 || (mapping_len > 0 && !laser_id_mapping))
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_upload_wire_frame: empty frame or bad layout") : LSA_E_ARG;
  if (mapping_len > kMaxRings) return ctx->fail(LSA_E_CAPACITY, "lsa_upload_wire_frame: more than 512 entries in the laser id mapping");
  const int offs[6] = {lay->off_x, lay->off_y, lay->off_z, lay->off_intensity, lay->off_time, lay->off_ring};
  for (int i = 0; i < 6; ++i)
    if (offs[i] < 0 || offs[i] + (i == 5 ? 2 : 4) > lay->point_step) return ctx->fail(LSA_E_ARG, "lsa_upload_wire_frame: field outside the record");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const unsigned char* raw = static_cast<const unsigned char*>(data);
  auto f32 = [&](int i, int off) { float v; std::memcpy(&v, raw + (size_t)i * lay->point_step + off, sizeof(v)); return v; };
  // "If first and last points have same timestamps, this is not normal" (VelodyneToLidarNode.cxx:74)
  const bool isTimeValid = f32(n - 1, lay->off_time) - f32(0, lay->off_time) > 1e-8;
  auto on_host = [&]() -> int {
    // host conversion (libm atan2 / fmod, ring by ring in arrival order, as the driver node does): the first frame,
    // whose azimuthal resolution is estimated on the host from the converted points anyway, and frames the device
    // cannot bucket by ring
    std::vector<lsa_point_t> pts(n);
    FrameAdvancementEstimator est;
    for (int i = 0; i < n; ++i)
    {
      lsa_point_t& p = pts[i];
      uint16_t ring;
      std::memcpy(&ring, raw + (size_t)i * lay->point_step + lay->off_ring, sizeof(ring));
      p.x = f32(i, lay->off_x); p.y = f32(i, lay->off_y); p.z = f32(i, lay->off_z); p.w = 1.f;
      p.intensity = f32(i, lay->off_intensity);
      p.laser_id = (uint16_t)mapped_laser_id(laser_id_mapping, mapping_len, ring, ring);
      p.device_id = (uint8_t)device_id;
      p.label = 0;
      if (isTimeValid) p.time = f32(i, lay->off_time);
      else
      {
        const double adv = est(p.x, p.y, p.laser_id);
        p.time = (timestamp_first_packet ? adv : adv - 1) / rpm * 60.;
      }
    }
    const int rc = lsa_upload_frame(ctx, pts.data(), n);
    if (rc) return rc;
    LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // pts goes away
    return LSA_OK;
  };
  if (ctx->az_res <= 0.f) return on_host();
  int rc = ensure_capacity(ctx, n);
  if (rc) return rc;
  LSA_HIP(ctx, frame_writer_guard(ctx, ctx->stream));  // frame_own is about to be rewritten: behind a dense-map insertion that reads it
  const size_t bytes = (size_t)n * lay->point_step;
  rc = ensure_scratch(ctx, bytes);
  if (rc) return rc;
  WireMap m;
  m.advancement = isTimeValid ? 0 : 1;
  m.lay = *lay;
  m.mapping_len = mapping_len;
  m.device_id = device_id;
  if (mapping_len > 0) std::memcpy(m.mapping, laser_id_mapping, (size_t)mapping_len * sizeof(uint16_t));
  LSA_HIP(ctx, hipMemcpyAsync(ctx->scratch_out, data, bytes, hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "wire_to_points", (double)n * (lay->point_step + 32));
    hipLaunchKernelGGL(k_wire_to_points, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, static_cast<const unsigned char*>(ctx->scratch_out), n, m,
                       reinterpret_cast<float4*>(ctx->frame_own));
  }
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's buffer may be pageable and go away
  if (!isTimeValid)
  {
    // no usable time field: built from the azimuth advancement (per ring, + 1 behind a descent until a NaN advancement
    // resets the ring: scanned on the ring-bucketed frame), on the device; laser ids the bucketing cannot hold go through
    // the host
    rc = time_from_advancement(ctx, ctx->frame_own, n, rpm, timestamp_first_packet);
    if (rc == LSA_E_CAPACITY) return on_host();
    if (rc) return rc;
  }
  ctx->frame = ctx->frame_own;
  ctx->frame_n = n;
  ctx->inbox_current = -1;
  return LSA_OK;
}

// ---- vtkSlam::PolyDataToPointCloud (paraview_wrapping/Plugin/vtkLidarSlam/vtkSlam.cxx:668-707) on the device -----------
namespace
{
struct SoaFrame
{
  const void* xyz; const void* time; const void* laser; const void* intensity;
  int xyz_type, time_type, laser_type, intensity_type;
  int n;
  int mapping_len;
  double factor;  // TimeToSecondsFactor
  uint16_t mapping[kMaxRings];
};
__device__ __forceinline__ double soa_value(const void* base, int type, size_t i)
{
  switch (type)
  {
    case LSA_SCALAR_F32: return (double)static_cast<const float*>(base)[i];
    case LSA_SCALAR_F64: return static_cast<const double*>(base)[i];
    case LSA_SCALAR_U8: return (double)static_cast<const unsigned char*>(base)[i];
    case LSA_SCALAR_U16: return (double)static_cast<const unsigned short*>(base)[i];
    case LSA_SCALAR_U32: return (double)static_cast<const unsigned int*>(base)[i];
    default: return (double)static_cast<const int*>(base)[i];
  }
}
__device__ __forceinline__ long long ordered_bits(double v)
{
  const long long b = __double_as_longlong(v);
  return b >= 0 ? b : b ^ 0x7fffffffffffffffll;
}
// frame end time = the largest value of the time array (arrayTime->GetRange()[1])
__global__ __launch_bounds__(256) void k_soa_scan_chunks(SoaFrame f, long long* __restrict__ tmax)
{
  __shared__ long long mx[4];
  long long m = (long long)0x8000000000000000ull;
  for (int q = 0; q < 4; ++q)
  {
    const int i = blockIdx.x * 1024 + q * 256 + threadIdx.x;
    if (i < f.n)
    {
      const long long t = ordered_bits(soa_value(f.time, f.time_type, i));
      m = t > m ? t : m;
    }
  }
  m = block_reduce<4>(m, OpMax(), mx);
  if (threadIdx.x == 0) atomicMax(tmax, m);
}
// points with all-zero coordinates are dropped
struct SoaKeep
{
  const void* xyz;
  int xyz_type;
  __device__ bool operator()(int i) const
  {
    const double x = soa_value(xyz, xyz_type, 3 * (size_t)i), y = soa_value(xyz, xyz_type, 3 * (size_t)i + 1), z = soa_value(xyz, xyz_type, 3 * (size_t)i + 2);
    return x != 0. || y != 0. || z != 0.;
  }
};
// the points that stay, in order, as LidarPoints: time relative to the frame's end [s], laser id (mapped), intensity
struct SoaEmit
{
  SoaFrame f;
  const long long* tmax;
  float4* out;
  __device__ void operator()(int i, int at) const
  {
    const long long tb = *tmax;
    const double end_time = __longlong_as_double(tb >= 0 ? tb : tb ^ 0x7fffffffffffffffll);
    const double x = soa_value(f.xyz, f.xyz_type, 3 * (size_t)i), y = soa_value(f.xyz, f.xyz_type, 3 * (size_t)i + 1), z = soa_value(f.xyz, f.xyz_type, 3 * (size_t)i + 2);
    const double t = (soa_value(f.time, f.time_type, i) - end_time) * f.factor;
    const double lid = soa_value(f.laser, f.laser_type, i);
    const unsigned id = mapped_laser_id(f.mapping, f.mapping_len, (size_t)lid, (unsigned)(unsigned short)lid);
    store_lidar_point(out, at, (float)x, (float)y, (float)z, t, (float)soa_value(f.intensity, f.intensity_type, i), id & 0xffffu, 0);  // device_id 0
  }
};
int scalar_size(int type) { return type == LSA_SCALAR_F64 ? 8 : type == LSA_SCALAR_U8 ? 1 : type == LSA_SCALAR_U16 ? 2 : 4; }
}  // namespace

int lsa_upload_polydata_frame(lsa_ctx* ctx, int n, const void* xyz, int xyz_type, const void* time, int time_type, const void* laser_id, int laser_type,
                              const void* intensity, int intensity_type, const uint16_t* laser_id_mapping, int mapping_len, double time_to_seconds,
                              uint64_t* stamp_us, int* n_valid)
{
  if (!ctx || n <= 0 || !xyz || !time || !laser_id || !intensity || mapping_len < 0 || (mapping_len > 0 && !laser_id_mapping) ||
      (xyz_type != LSA_SCALAR_F32 && xyz_type != LSA_SCALAR_F64))
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_upload_polydata_frame: bad argument") : LSA_E_ARG;
  for (int t : {time_type, laser_type, intensity_type})
    if (t < LSA_SCALAR_F32 || t > LSA_SCALAR_I32) return ctx->fail(LSA_E_ARG, "lsa_upload_polydata_frame: unknown scalar type");
  if (mapping_len > kMaxRings) return ctx->fail(LSA_E_CAPACITY, "lsa_upload_polydata_frame: more than 512 entries in the laser id mapping");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure_capacity(ctx, n);
  if (rc) return rc;
  LSA_HIP(ctx, frame_writer_guard(ctx, ctx->stream));  // frame_own is about to be rewritten: behind a dense-map insertion that reads it
  // the four arrays go to the device as they are (structure of arrays, no LidarPoint cloud is built on the host)
  const size_t sz[4] = {(size_t)3 * n * scalar_size(xyz_type), (size_t)n * scalar_size(time_type), (size_t)n * scalar_size(laser_type),
                        (size_t)n * scalar_size(intensity_type)};
  size_t off[4], total = 0;
  for (int i = 0; i < 4; ++i) { off[i] = total; total += (sz[i] + 255) / 256 * 256; }
  const int nchunks = (n + 1023) / 1024;
  const size_t off_counts = total, off_tmax = off_counts + ((size_t)(nchunks + 1) * sizeof(int) + 255) / 256 * 256;
  rc = ensure_scratch(ctx, off_tmax + 64);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch_out);
  const void* src[4] = {xyz, time, laser_id, intensity};
  for (int i = 0; i < 4; ++i) LSA_HIP(ctx, hipMemcpyAsync(base + off[i], src[i], sz[i], hipMemcpyHostToDevice, ctx->stream));
  SoaFrame f;
  f.xyz = base + off[0]; f.time = base + off[1]; f.laser = base + off[2]; f.intensity = base + off[3];
  f.xyz_type = xyz_type; f.time_type = time_type; f.laser_type = laser_type; f.intensity_type = intensity_type;
  f.n = n;
  f.mapping_len = mapping_len;
  f.factor = time_to_seconds;
  if (mapping_len > 0) std::memcpy(f.mapping, laser_id_mapping, (size_t)mapping_len * sizeof(uint16_t));
  int* counts = reinterpret_cast<int*>(base + off_counts);
  long long* tmax = reinterpret_cast<long long*>(base + off_tmax);
  const long long lowest = (long long)0x8000000000000000ull;
  LSA_HIP(ctx, hipMemcpyAsync(tmax, &lowest, sizeof(lowest), hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "polydata_to_points", (double)total + (double)n * 32);
    hipLaunchKernelGGL(k_soa_scan_chunks, dim3(nchunks), dim3(256), 0, ctx->stream, f, tmax);
    stable_compact(ctx->stream, counts, nullptr, SoaKeep{f.xyz, xyz_type}, SoaEmit{f, tmax, reinterpret_cast<float4*>(ctx->frame_own)}, nullptr, n, counts + nchunks);
  }
  long long tb = 0;
  int kept = 0;
  LSA_HIP(ctx, hipMemcpyAsync(&tb, tmax, sizeof(tb), hipMemcpyDeviceToHost, ctx->stream));
  rc = adopt_compacted_frame(ctx, counts + nchunks, &kept);  // waits: the caller's arrays may go away; stamp and size are needed now
  if (rc) return rc;
  tb = tb >= 0 ? tb : tb ^ 0x7fffffffffffffffll;
  double end_time;
  std::memcpy(&end_time, &tb, sizeof(end_time));
  if (stamp_us) *stamp_us = (uint64_t)(end_time * (time_to_seconds * 1e6));  // pc->header.stamp = frameEndTime * (factor * 1e6) (:683)
  if (n_valid) *n_valid = kept;
  return kept == n ? 1 : 0;  // allPointsAreValid
}

// ---- RobosenseToLidarNode::Callback (ros_wrapping/lidar_conversions/src/RobosenseToLidarNode.cxx:58-125) on the device ----
namespace
{
struct RsFrame
{
  const unsigned char* raw;
  int step, off_x, off_y, off_z, off_i;
  int n, width, points_per_ring, nlasers;
  int mapping_len, device_id;
  double rpm;
  uint16_t mapping[kMaxRings];
};
__device__ __forceinline__ float rs_f32(const RsFrame& f, int i, int off) { return *reinterpret_cast<const float*>(f.raw + (size_t)i * f.step + off); }
__device__ __forceinline__ bool rs_finite(const RsFrame& f, int i) { return isfinite(rs_f32(f, i, f.off_x)) && isfinite(rs_f32(f, i, f.off_y)) && isfinite(rs_f32(f, i, f.off_z)); }
// the last record with finite coordinates of every chunk of 1024 (-1: none)
__global__ __launch_bounds__(256) void k_rs_last_finite(RsFrame f, int* __restrict__ chunk_last)
{
  __shared__ int last;
  if (threadIdx.x == 0) last = -1;
  __syncthreads();
  int mine = -1;
  for (int q = 0; q < 4; ++q)
  {
    const int i = blockIdx.x * 1024 + q * 256 + threadIdx.x;
    if (i < f.n && rs_finite(f, i)) mine = i;
  }
  if (mine >= 0) atomicMax(&last, mine);
  __syncthreads();
  if (threadIdx.x == 0) chunk_last[blockIdx.x] = last;
}
// chunk_last -> the last finite record IN FRONT of every chunk (exclusive running maximum; one block)
__global__ __launch_bounds__(1024) void k_rs_carry(int* __restrict__ chunk_last, int nchunks)
{
  __shared__ int s[1024];
  int run = -1;
  for (int base = 0; base < nchunks; base += 1024)
  {
    const int i = base + threadIdx.x;
    const int v = i < nchunks ? chunk_last[i] : -1;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1)
    {
      const int a = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : -1;
      __syncthreads();
      s[threadIdx.x] = max(s[threadIdx.x], a);
      __syncthreads();
    }
    const int before = threadIdx.x > 0 ? s[threadIdx.x - 1] : -1;
    if (i < nchunks) chunk_last[i] = max(run, before);
    run = max(run, s[1023]);
    __syncthreads();
  }
}
// A record stays when its coordinates are finite and differ from those of the last point KEPT.  A record skipped as a
// duplicate has the coordinates of the point kept before it, so "the last point kept" and "the nearest finite record in
// front" have the same coordinates: no sequential pass is needed.  keep[i].
__global__ __launch_bounds__(256) void k_rs_keep(RsFrame f, const int* __restrict__ chunk_carry, uint8_t* __restrict__ keep)
{
  __shared__ uint8_t fin[1024];
  const int c0 = blockIdx.x * 1024;
  for (int q = 0; q < 4; ++q)
  {
    const int l = q * 256 + threadIdx.x, i = c0 + l;
    fin[l] = (i < f.n && rs_finite(f, i)) ? 1 : 0;
  }
  __syncthreads();
  for (int q = 0; q < 4; ++q)
  {
    const int l = q * 256 + threadIdx.x, i = c0 + l;
    if (i >= f.n) continue;
    bool k = false;
    if (fin[l])
    {
      int j = l - 1;
      while (j >= 0 && !fin[j]) --j;
      const int prev = j >= 0 ? c0 + j : chunk_carry[blockIdx.x];
      k = prev < 0 || !(rs_f32(f, i, f.off_x) == rs_f32(f, prev, f.off_x) && rs_f32(f, i, f.off_y) == rs_f32(f, prev, f.off_y) &&
                        rs_f32(f, i, f.off_z) == rs_f32(f, prev, f.off_z));
    }
    keep[i] = k ? 1 : 0;
  }
}
struct RsKeep { const uint8_t* keep; __device__ bool operator()(int i) const { return keep[i]; } };
// the points that stay, in order, as LidarPoints
struct RsEmit
{
  RsFrame f;
  float4* out;
  __device__ void operator()(int i, int at) const
  {
    const unsigned ring = (unsigned)i / (unsigned)f.width;
    // LaserIdMapping if given, RS16's when the input has 16 rings, otherwise the ring itself (:106-109)
    const unsigned rs16 = ring < 8u ? ring : 23u - ring;  // {0..7, 15, 14, ..., 8}
    const unsigned id = mapped_laser_id(f.mapping, f.mapping_len, ring, f.nlasers == 16 ? rs16 : ring);
    const double adv = (double)((unsigned)i % (unsigned)f.points_per_ring) / (double)f.points_per_ring;
    const double t = (adv - 1) / f.rpm * 60.;
    store_lidar_point(out, at, rs_f32(f, i, f.off_x), rs_f32(f, i, f.off_y), rs_f32(f, i, f.off_z), t, rs_f32(f, i, f.off_i), id & 0xffffu, f.device_id);
  }
};
}  // namespace

int lsa_upload_robosense_frame(lsa_ctx* ctx, const void* records, int width, int height, const lsa_wire_layout_t* lay, const uint16_t* laser_id_mapping,
                               int mapping_len, int device_id, double rpm, int* n_valid)
{
  if (!ctx || !records || !lay || width <= 0 || height <= 0 || lay->point_step <= 0 || mapping_len < 0 || (mapping_len > 0 && !laser_id_mapping) || !(rpm > 0.) ||
      (long long)width * height > (1ll << 30))
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_upload_robosense_frame: empty frame or bad layout") : LSA_E_ARG;
  if (mapping_len > kMaxRings) return ctx->fail(LSA_E_CAPACITY, "lsa_upload_robosense_frame: more than 512 entries in the laser id mapping");
  if (mapping_len > 0 && mapping_len < height) return ctx->fail(LSA_E_ARG, "lsa_upload_robosense_frame: the laser id mapping is shorter than the cloud is high");
  const int offs[4] = {lay->off_x, lay->off_y, lay->off_z, lay->off_intensity};
  for (int o : offs)
    if (o < 0 || o + 4 > lay->point_step || (o & 3)) return ctx->fail(LSA_E_ARG, "lsa_upload_robosense_frame: field outside the record or not aligned");
  if (lay->point_step & 3) return ctx->fail(LSA_E_ARG, "lsa_upload_robosense_frame: records must be a multiple of 4 bytes");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const int n = width * height;
  int rc = ensure_capacity(ctx, n);
  if (rc) return rc;
  LSA_HIP(ctx, frame_writer_guard(ctx, ctx->stream));  // frame_own is about to be rewritten: behind a dense-map insertion that reads it
  const size_t bytes = (size_t)n * lay->point_step;
  const int nchunks = (n + 1023) / 1024;
  const size_t off_keep = (bytes + 255) / 256 * 256, off_last = off_keep + ((size_t)n + 255) / 256 * 256,
               off_counts = off_last + ((size_t)nchunks * sizeof(int) + 255) / 256 * 256;
  rc = ensure_scratch(ctx, off_counts + (size_t)(nchunks + 1) * sizeof(int) + 64);
  if (rc) return rc;
  char* base = static_cast<char*>(ctx->scratch_out);
  LSA_HIP(ctx, hipMemcpyAsync(base, records, bytes, hipMemcpyHostToDevice, ctx->stream));
  RsFrame f;
  f.raw = reinterpret_cast<const unsigned char*>(base);
  f.step = lay->point_step; f.off_x = lay->off_x; f.off_y = lay->off_y; f.off_z = lay->off_z; f.off_i = lay->off_intensity;
  f.n = n; f.width = width; f.nlasers = height; f.points_per_ring = n / height;
  f.mapping_len = mapping_len; f.device_id = device_id; f.rpm = rpm;
  if (mapping_len > 0) std::memcpy(f.mapping, laser_id_mapping, (size_t)mapping_len * sizeof(uint16_t));
  uint8_t* keep = reinterpret_cast<uint8_t*>(base + off_keep);
  int* last = reinterpret_cast<int*>(base + off_last);
  int* counts = reinterpret_cast<int*>(base + off_counts);
  {
    ProfScope ps(ctx, "robosense_to_points", (double)bytes + (double)n * 32);
    hipLaunchKernelGGL(k_rs_last_finite, dim3(nchunks), dim3(256), 0, ctx->stream, f, last);
    hipLaunchKernelGGL(k_rs_carry, dim3(1), dim3(1024), 0, ctx->stream, last, nchunks);
    hipLaunchKernelGGL(k_rs_keep, dim3(nchunks), dim3(256), 0, ctx->stream, f, last, keep);
    stable_compact(ctx->stream, counts, nullptr, RsKeep{keep}, RsEmit{f, reinterpret_cast<float4*>(ctx->frame_own)}, nullptr, n, counts + nchunks);
  }
  return adopt_compacted_frame(ctx, counts + nchunks, n_valid);  // waits: the caller's records may go away; the size is needed now
}

}  // extern "C"
