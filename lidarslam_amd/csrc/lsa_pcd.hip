// lsa_pcd.hip -- the keypoint maps between PCD files and the device grids (Slam::SaveMapsToPCD / LoadMapsFromPCD,
// slam_lib/src/Slam.cxx:504-543): the conversion between a file's record layout and the 32-byte LidarPoint runs on the
// device, next to where the points live; the host reads or writes the file and, for the two formats that need it, parses
// text or runs the LZF stage (host/lsa_pcd.cpp).
//
// Load: the data section goes up in pieces of kPieceBytes -- the host fills one pinned piece while the copy stream sends
// the other and k_pcd_decode, on the grid's stream, converts the one before into the grid's batch buffer -- and the grid
// then takes the whole file as ONE Add (the reference rolls once to the whole cloud's box, applies the sampling rule in
// arrival order and counts one frame per voxel per call, RollingGrid.cxx:117-318).
// Save: RollingGrid::Get stays on the device (grid_collect), k_pcd_encode writes packed records or the eight columns
// straight into the pinned pieces, the host assembles, compresses and writes.
//
// Both kernels stream: one thread per point, 28 + 32 bytes of traffic each.  Two forms of the record side, chosen by
// measurement: lanes touching the records directly (byte loads of any offset / seven word stores at a
// 28-byte stride) and a workgroup staging its 256 records through LDS with whole-word, coalesced accesses.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <new>
#include "lsa_device_grid_io.h"
#include "host/lsa_pcd.h"

using namespace lsa;

namespace
{
constexpr size_t kPieceBytes = 8u << 20;
constexpr int kBlock = 256;
constexpr int kLdsStrideMax = 128;  // records of up to 128 bytes are staged through LDS (32 KiB a workgroup)
constexpr int kLdsDefault = 1;      // the form of the record side in use: through LDS, the faster one (lsa_debug_set "pcd_lds" picks the other for a comparison)

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

__device__ inline void store_point(lsa_point_t* dst, const lsa_point_t& p)
{
  float4 v[2];
  memcpy(v, &p, sizeof(p));
  float4* d = reinterpret_cast<float4*>(dst);
  d[0] = v[0];
  d[1] = v[1];
}

// The table travels by value in the kernel arguments and is only read (a written or aliased argument struct is copied to
// scratch memory).  `data`: a piece's records, or its columns one after the other.
__global__ __launch_bounds__(kBlock) void k_pcd_decode(const unsigned char* __restrict__ data, const pcd::ColumnTable table, int n, lsa_point_t* __restrict__ out)
{
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  store_point(out + i, pcd::decode_point(data, table, i));
}

// the same for records of `stride` bytes (stride * kBlock bytes of dynamic LDS): the workgroup's records are one contiguous,
// word-aligned span, loaded with whole words by consecutive lanes; the fields are then assembled from LDS bytes
__global__ __launch_bounds__(kBlock) void k_pcd_decode_lds(const unsigned char* __restrict__ data, const pcd::ColumnTable table, int n, int stride, lsa_point_t* __restrict__ out)
{
  extern __shared__ uint32_t lds_words[];
  const int first = blockIdx.x * kBlock;
  const int here = min(kBlock, n - first);
  const int words = (here * stride + 3) / 4;  // (the piece's device buffer has room for the last word's spare bytes)
  const uint32_t* src = reinterpret_cast<const uint32_t*>(data + (size_t)first * stride);  // first * stride is a multiple of 4
  for (int w = threadIdx.x; w < words; w += kBlock) lds_words[w] = src[w];
  __syncthreads();
  if ((int)threadIdx.x >= here) return;
  store_point(out + first + threadIdx.x, pcd::decode_point(reinterpret_cast<const unsigned char*>(lds_words), table, threadIdx.x));
}

__device__ inline lsa_point_t load_point(const lsa_point_t* src)
{
  const float4* s = reinterpret_cast<const float4*>(src);
  float4 v[2] = {s[0], s[1]};
  lsa_point_t p;
  memcpy(&p, v, sizeof(p));
  return p;
}

// n points into packed 28-byte records (columns == 0) or into the eight columns of n points, field after field
__global__ __launch_bounds__(kBlock) void k_pcd_encode(const lsa_point_t* __restrict__ pts, int n, int columns, unsigned char* __restrict__ out)
{
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t w[7];
  pcd::encode_record(load_point(pts + i), w);
  uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
  if (!columns)
  {
    for (int k = 0; k < 7; ++k) o32[(size_t)i * 7 + k] = w[k];
    return;
  }
  const size_t N = (size_t)n;
  o32[i] = w[0];
  o32[N + i] = w[1];
  o32[2 * N + i] = w[2];
  o32[3 * N + 2 * (size_t)i] = w[3];  // time: two words, the column starts at 12 n bytes, not always a multiple of 8
  o32[3 * N + 2 * (size_t)i + 1] = w[4];
  o32[5 * N + i] = w[5];
  reinterpret_cast<uint16_t*>(out + 24 * N)[i] = (uint16_t)w[6];
  out[26 * N + i] = (unsigned char)(w[6] >> 16);
  out[27 * N + i] = (unsigned char)(w[6] >> 24);
}

// the record form through LDS: every lane leaves its seven words (stride 7: no bank conflict), the workgroup writes the
// 1792 words of its 256 records by consecutive lanes
__global__ __launch_bounds__(kBlock) void k_pcd_encode_lds(const lsa_point_t* __restrict__ pts, int n, unsigned char* __restrict__ out)
{
  __shared__ uint32_t lds_words[kBlock * 7];
  const int first = blockIdx.x * kBlock;
  const int here = min(kBlock, n - first);
  if ((int)threadIdx.x < here)
  {
    uint32_t w[7];
    pcd::encode_record(load_point(pts + first + threadIdx.x), w);
    for (int k = 0; k < 7; ++k) lds_words[threadIdx.x * 7 + k] = w[k];
  }
  __syncthreads();
  uint32_t* dst = reinterpret_cast<uint32_t*>(out) + (size_t)first * 7;
  for (int w = threadIdx.x; w < here * 7; w += kBlock) dst[w] = lds_words[w];
}

int ensure_pieces(lsa_ctx* ctx)
{
  if (ctx->pcd_piece) return LSA_OK;
  for (int b = 0; b < 2; ++b)
  {
    LSA_HIP(ctx, hipHostMalloc(&ctx->pcd_pinned[b], kPieceBytes, hipHostMallocDefault));
    LSA_HIP(ctx, hipMalloc(&ctx->pcd_dev[b], kPieceBytes + 16));
    LSA_HIP(ctx, hipEventCreateWithFlags(&ctx->pcd_ev_copy[b], hipEventDisableTiming));
    LSA_HIP(ctx, hipEventCreateWithFlags(&ctx->pcd_ev_kernel[b], hipEventDisableTiming));
  }
  ctx->pcd_piece = kPieceBytes;
  return LSA_OK;
}

struct FileCloser
{
  FILE* f = nullptr;
  ~FileCloser() { if (f) std::fclose(f); }
};

// However a load leaves its loop of pieces -- a short read, a HIP error -- the copies it has enqueued have left the pinned
// pieces before anybody fills them again (the next load starts filling both without a wait).
struct CopyDrain
{
  hipStream_t stream;
  ~CopyDrain() { (void)hipStreamSynchronize(stream); }
};
}  // namespace

extern "C" {

// RollingGrid::Add(cloud of the file, fixed, time, roll_first) without the cloud ever being a LidarPoint cloud on the host
static int add_pcd(lsa_device_grid* g, const char* path, int fixed, double time, int roll_first);
static int save_pcd(lsa_device_grid* g, const char* path, int format, int clean);

// (no exception crosses the C boundary: a file too large for the host's memory is an error like any other)
int lsa_device_grid_add_pcd(lsa_device_grid* g, const char* path, int fixed, double time, int roll_first)
{
  if (!g) return LSA_E_ARG;
  try { return add_pcd(g, path, fixed, time, roll_first); }
  catch (const std::bad_alloc&) { return grid_context(g)->fail(LSA_E_CAPACITY, std::string(path ? path : "") + ": not enough host memory"); }
}
int lsa_device_grid_save_pcd(lsa_device_grid* g, const char* path, int format, int clean)
{
  if (!g) return LSA_E_ARG;
  try { return save_pcd(g, path, format, clean); }
  catch (const std::bad_alloc&) { return grid_context(g)->fail(LSA_E_CAPACITY, std::string(path ? path : "") + ": not enough host memory"); }
}

static int add_pcd(lsa_device_grid* g, const char* path, int fixed, double time, int roll_first)
{
  lsa_ctx* ctx = grid_context(g);
  if (!path) return ctx->fail(LSA_E_ARG, "lsa_device_grid_add_pcd: no path");
  pcd::Cloud cloud;
  std::string err;
  int rc = pcd::read_cloud(path, cloud, err, false);
  if (rc) return ctx->fail(rc, err);
  const pcd::Header& h = cloud.header;
  const int n = (int)h.points;
  double* T = ctx->pcd_times;
  std::fill(T, T + 8, 0.);
  T[0] = pcd::timing().file; T[1] = pcd::timing().lzf; T[2] = pcd::timing().text; T[6] = n;
  if (n == 0) return LSA_OK;  // "Pointcloud is empty, voxel grid not updated."
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  lsa_point_t* batch = nullptr;
  rc = grid_batch(g, n, &batch);
  if (!rc) rc = ensure_pieces(ctx);
  if (rc) return rc;
  hipStream_t gs = grid_stream(g);

  // what a piece carries per point: its record, or the values of the columns in use
  int used[pcd::kNbFields], nused = 0, per_point = 0;
  if (cloud.columns)
  {
    for (int k = 0; k < pcd::kNbFields; ++k)
      if (cloud.table.c[k].type != pcd::kAbsent) { used[nused++] = k; per_point += cloud.table.c[k].size; }
    if (nused == 0) per_point = 1;
  }
  else per_point = h.record_bytes;
  if (per_point <= 0) return ctx->fail(LSA_E_ARG, std::string(path) + ": records of no bytes");
  if ((size_t)per_point > kPieceBytes) return ctx->fail(LSA_E_CAPACITY, std::string(path) + ": records of more than 8 MiB");
  int per_piece = (int)(kPieceBytes / per_point);
  if (per_piece > kBlock) per_piece -= per_piece % kBlock;
  const bool streamed = h.format == pcd::kBinary;  // the records come from the file piece by piece
  FileCloser file;
  if (streamed)
  {
    file.f = std::fopen(path, "rb");
    if (!file.f || std::fseek(file.f, (long)h.data_offset, SEEK_SET) != 0) return ctx->fail(LSA_E_ARG, std::string(path) + ": cannot be read");
  }
  const bool lds = !cloud.columns && h.record_bytes <= kLdsStrideMax && h.record_bytes % 4 == 0 && (ctx->pcd_lds < 0 ? kLdsDefault : ctx->pcd_lds) != 0;
  const double t_begin = now_s();
  double t_file = 0;
  CopyDrain drain{ctx->copy_stream};
  for (int p0 = 0, piece = 0; p0 < n; p0 += per_piece, ++piece)
  {
    const int b = piece & 1;
    const int cnt = std::min(per_piece, n - p0);
    unsigned char* pin = static_cast<unsigned char*>(ctx->pcd_pinned[b]);
    if (piece >= 2) LSA_HIP(ctx, hipEventSynchronize(ctx->pcd_ev_copy[b]));  // the copy out of this pinned piece is over
    pcd::ColumnTable t = cloud.table;
    size_t bytes = 0;
    if (cloud.columns)
    {
      for (int u = 0; u < nused; ++u)
      {
        pcd::Column& c = t.c[used[u]];
        std::memcpy(pin + bytes, cloud.data.data() + c.base + (size_t)p0 * c.size, (size_t)cnt * c.size);
        c.base = (int64_t)bytes;
        bytes += (size_t)cnt * c.size;
      }
    }
    else
    {
      bytes = (size_t)cnt * h.record_bytes;
      if (streamed)
      {
        const double t0 = now_s();
        if (std::fread(pin, 1, bytes, file.f) != bytes)
          return ctx->fail(LSA_E_ARG, std::string(path) + ":" + std::to_string(h.data_line) + ": the data section is truncated: " + std::to_string((size_t)n * h.record_bytes) + " bytes expected");
        t_file += now_s() - t0;
      }
      else std::memcpy(pin, cloud.data.data() + (size_t)p0 * h.record_bytes, bytes);
    }
    LSA_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->pcd_ev_kernel[b], 0));  // the kernel that read this device piece last (an earlier load's, too) is over
    {
      ProfScope ps(ctx, "pcd_upload", (double)bytes, ctx->copy_stream);
      LSA_HIP(ctx, hipMemcpyAsync(ctx->pcd_dev[b], pin, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
    }
    LSA_HIP(ctx, hipEventRecord(ctx->pcd_ev_copy[b], ctx->copy_stream));
    LSA_HIP(ctx, hipStreamWaitEvent(gs, ctx->pcd_ev_copy[b], 0));
    {
      ProfScope ps(ctx, "pcd_decode", (double)bytes + (double)cnt * sizeof(lsa_point_t), gs);
      const unsigned char* src = static_cast<const unsigned char*>(ctx->pcd_dev[b]);
      const dim3 grid((cnt + kBlock - 1) / kBlock);
      if (lds) hipLaunchKernelGGL(k_pcd_decode_lds, grid, dim3(kBlock), (size_t)kBlock * h.record_bytes, gs, src, t, cnt, h.record_bytes, batch + p0);
      else hipLaunchKernelGGL(k_pcd_decode, grid, dim3(kBlock), 0, gs, src, t, cnt, batch + p0);
    }
    LSA_HIP(ctx, hipEventRecord(ctx->pcd_ev_kernel[b], gs));
  }
  // a failed copy is reported here
  LSA_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
  if (ctx->profiling) LSA_HIP(ctx, hipStreamSynchronize(gs));
  if (streamed) T[0] = t_file;
  T[3] = now_s() - t_begin;
  T[5] = (double)n * per_point;
  const double t_add = now_s();
  rc = grid_add_batch(g, n, fixed != 0, time, roll_first != 0);
  if (rc) return rc;
  if (ctx->profiling) LSA_HIP(ctx, hipStreamSynchronize(gs));
  T[4] = now_s() - t_add;
  return LSA_OK;
}

// RollingGrid::Get(clean) into a PCD file: the number of points written; 0 and no file when the map hands out no point
// (an empty cloud is not saved, PointCloudStorage.h:91-92) -- told apart from every failure, which is negative
static int save_pcd(lsa_device_grid* g, const char* path, int format, int clean)
{
  lsa_ctx* ctx = grid_context(g);
  if (!path) return ctx->fail(LSA_E_ARG, "lsa_device_grid_save_pcd: no path");
  if (format < pcd::kAscii || format > pcd::kBinaryCompressed) return ctx->fail(-4, std::string(path) + ": unknown PCD format " + std::to_string(format));
  double* T = ctx->pcd_times;
  std::fill(T, T + 8, 0.);
  const double t_get = now_s();
  const lsa_point_t* pts = nullptr;
  int n = 0;
  int rc = grid_collect(g, clean, &pts, &n);
  if (rc) return rc;
  T[4] = now_s() - t_get;
  return lsa::pcd_save_device_points(ctx, grid_stream(g), pts, n, path, format);
}
}  // extern "C"

// n LidarPoints on the device (what kernels on `gs` left) into a PCD file: the part of a save that comes behind the collection,
// for the keypoint maps above and the dense map (lsa_dense_export.hip, lsa_dense_normals.hip).  The caller has checked path and format and set T[4].
// normals4 (host, may be null): n x 4 floats the writer puts behind every point -- interleaved on the host, the path is not hot.
int lsa::pcd_save_device_points(lsa_ctx* ctx, hipStream_t gs, const lsa_point_t* pts, int n, const char* path, int format, const float* normals4)
{
  double* T = ctx->pcd_times;
  T[6] = n;
  if (n == 0) return 0;
  int rc = ensure_pieces(ctx);
  if (rc) return rc;
  const bool columns = format == pcd::kBinaryCompressed;
  const bool lds = !columns && (ctx->pcd_lds < 0 ? kLdsDefault : ctx->pcd_lds) != 0;
  int per_piece = (int)(kPieceBytes / pcd::kRecordBytes);
  per_piece -= per_piece % kBlock;
  std::vector<unsigned char> raw((size_t)n * pcd::kRecordBytes);
  static const int sizes[pcd::kNbFields] = {4, 4, 4, 8, 4, 2, 1, 1};
  const double t_begin = now_s();
  // piece i is taken from its pinned buffer while the kernel writes piece i + 1 into the other
  auto take = [&](int piece) -> int {
    const int b = piece & 1, p0 = piece * per_piece, cnt = std::min(per_piece, n - p0);
    LSA_HIP(ctx, hipEventSynchronize(ctx->pcd_ev_kernel[b]));
    const unsigned char* pin = static_cast<const unsigned char*>(ctx->pcd_pinned[b]);
    if (!columns) std::memcpy(raw.data() + (size_t)p0 * pcd::kRecordBytes, pin, (size_t)cnt * pcd::kRecordBytes);
    else
    {
      size_t column = 0, from = 0;
      for (int k = 0; k < pcd::kNbFields; ++k)
      {
        std::memcpy(raw.data() + column + (size_t)p0 * sizes[k], pin + from, (size_t)cnt * sizes[k]);
        column += (size_t)n * sizes[k];
        from += (size_t)cnt * sizes[k];
      }
    }
    return LSA_OK;
  };
  int pieces = 0;
  for (int p0 = 0; p0 < n; p0 += per_piece, ++pieces)
  {
    const int b = pieces & 1, cnt = std::min(per_piece, n - p0);
    {
      ProfScope ps(ctx, "pcd_encode", (double)cnt * (sizeof(lsa_point_t) + pcd::kRecordBytes), gs);
      unsigned char* dst = static_cast<unsigned char*>(ctx->pcd_pinned[b]);
      const dim3 grid((cnt + kBlock - 1) / kBlock);
      if (lds) hipLaunchKernelGGL(k_pcd_encode_lds, grid, dim3(kBlock), 0, gs, pts + p0, cnt, dst);
      else hipLaunchKernelGGL(k_pcd_encode, grid, dim3(kBlock), 0, gs, pts + p0, cnt, columns ? 1 : 0, dst);
    }
    LSA_HIP(ctx, hipEventRecord(ctx->pcd_ev_kernel[b], gs));
    if (pieces > 0 && (rc = take(pieces - 1)) != LSA_OK) return rc;
  }
  if ((rc = take(pieces - 1)) != LSA_OK) return rc;
  T[3] = now_s() - t_begin;
  T[5] = (double)n * (pcd::kRecordBytes + (normals4 ? pcd::kNormalBytes : 0));
  std::string err;
  rc = pcd::write_records(path, columns ? nullptr : raw.data(), columns ? raw.data() : nullptr, n, format, err, normals4);
  T[0] = pcd::timing().file; T[1] = pcd::timing().lzf; T[2] = pcd::timing().text;
  if (rc) return ctx->fail(rc, err);
  return n;
}

extern "C" {
// Seconds of the last lsa_device_grid_add_pcd / _save_pcd of the context (diagnostics): [0] file, [1] LZF, [2] text,
// [3] pieces on their way (upload + conversion, overlapped), [4] the grid's Add / Get, [5] bytes moved, [6] points.
// [3] and [4] wait for the device only while profiling is on; otherwise they are the time to enqueue.
int lsa_pcd_io_times(const lsa_ctx* ctx, double out[8])
{
  if (!ctx || !out) return LSA_E_ARG;
  std::copy(ctx->pcd_times, ctx->pcd_times + 8, out);
  return LSA_OK;
}

}  // extern "C"
