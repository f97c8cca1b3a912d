// lsa_kplog.hip -- the keypoint log in HBM and its replay under a corrected trajectory.
//   the log        Slam::LogCurrentFrameState (slam_lib/src/Slam.cxx:1225-1255): CurrentRawKeypoints[k] of every logged pose,
//                  the oldest frame dropped whenever LogTrajectory drops its oldest pose
//   k_log_replay   the re-projection of Slam::RunPoseGraphOptimization (Slam.cxx:416-452): every logged frame's keypoints
//                  under the new poses, frame i >= 1 with the LinearTransformInterpolator between pose[i-1] and pose[i]
//                  (SetTimes(t[i] - t[i-1], 0.), evaluated at the point's own time) when undistortion is on, frame 0 and
//                  everything otherwise with the rigid pose[i]; and the box of the LAST frame's points (:472-475)
//   k_log_replay_range  the same for a range of frames, under one of three time rules, with the box of ALL replayed points:
//                  what the registration of logged frames (host/lsa_slam_log.cpp, RegisterLoggedFrames) makes its target
//                  sub-map and its query keypoints of
// Storage: an arena of fixed-size chunks.  A frame (its three types, one after the other) never straddles two chunks, so
// growth never copies; a chunk whose frames have all been popped goes to a free list; nothing is freed while work may be in
// flight (the context's graveyard, lsa_ctx.h).  The host keeps the frame table {device pointer, count} per frame and type.
// Slam::LoggingStorage: all five PointCloudStorageType values mean the same thing here -- uncompressed LidarPoints in HBM.
#include <algorithm>
#include <cfloat>
#include "lsa_ctx.h"
#include "lsa_device_math.h"
#include "lsa_device_grid_io.h"
#include "lsa_kplog_io.h"
#include "lsa_wave.h"

using namespace lsa;

namespace lsa
{
InterpConst make_interp_const(const double H0[16], const double H1[16], double t0, double t1);  // lsa_transform.hip

struct KpLogChunk
{
  char* base = nullptr;
  size_t bytes = 0, used = 0;
  int live = 0;  // frames that have points in it
};
struct KpLogFrame
{
  lsa_point_t* pts[3] = {nullptr, nullptr, nullptr};
  int n[3] = {0, 0, 0};
  int chunk = -1;  // -1: a frame without keypoints
};
struct KpLog
{
  std::vector<KpLogChunk> chunks;
  std::vector<int> free_list;  // chunks of the standard size without a live frame, kept for reuse
  std::deque<KpLogFrame> frames;
  int cur = -1;          // the chunk being filled
  bool stopped = false;  // a chunk could not be allocated: nothing is logged until lsa_kplog_clear
  size_t held = 0;       // bytes of all chunks, the free list included
  // replay: the per-frame tables on the device, the boxes' words, pinned staging for the host maps
  void* table = nullptr;
  size_t table_cap = 0;
  unsigned* box_dev = nullptr;
  lsa_point_t* stage[3] = {nullptr, nullptr, nullptr};
  long long stage_cap[3] = {0, 0, 0}, stage_n[3] = {0, 0, 0};
};

void kplog_destroy(lsa_ctx* ctx)
{
  KpLog* log = ctx->kplog;
  place_destroy(ctx);
  if (!log) return;
  for (KpLogChunk& c : log->chunks)
    if (c.base) (void)hipFree(c.base);
  if (log->table) (void)hipFree(log->table);
  if (log->box_dev) (void)hipFree(log->box_dev);
  for (int k = 0; k < 3; ++k)
    if (log->stage[k]) (void)hipHostFree(log->stage[k]);
  delete log;
  ctx->kplog = nullptr;
}

bool kplog_frame(const lsa_ctx* ctx, int frame, const lsa_point_t* pts[3], int n[3])
{
  const KpLog* log = ctx ? ctx->kplog : nullptr;
  if (!log || frame < 0 || frame >= (int)log->frames.size()) return false;
  for (int k = 0; k < 3; ++k) { pts[k] = log->frames[frame].pts[k]; n[k] = log->frames[frame].n[k]; }
  return true;
}
}  // namespace lsa

namespace
{
constexpr size_t kAlign = 256;
inline size_t aligned(size_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

__device__ __forceinline__ double point_time(const float4& b) { return __hiloint2double(__float_as_int(b.y), __float_as_int(b.x)); }

// the append: the three raw keypoint sets of a frame into their places in a chunk (blockIdx.y = type)
struct AppendArgs
{
  const float4* in[3];
  float4* out[3];
  int n[3];
};
__global__ __launch_bounds__(256) void k_log_append(AppendArgs s)
{
  const int t = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n[t]) return;
  s.out[t][2 * (size_t)i] = s.in[t][2 * (size_t)i];
  s.out[t][2 * (size_t)i + 1] = s.in[t][2 * (size_t)i + 1];
}

// what a frame's points are moved by: the constants k_undistort takes per launch (make_interp_const), or the rigid pose
struct FrameMotion
{
  InterpConst c;
  Rigid R;
  int interp;
  int pad;
};
struct ReplayArgs
{
  const FrameMotion* motion;     // [nframes]
  const long long* off[3];       // [nframes + 1] per type: points of that type in the frames before
  const float4* const* src[3];   // [nframes] per type: the frame's points in the log
  float4* out[3];                // frames ascending, inside a frame the logged order
  long long total[3];
  int nframes;
};
// The replayed point: which frame i lies in (one binary search in the offsets for the wavefront's first point, the lanes walk
// on from there: a frame has hundreds of points, an empty one is stepped over), the point moved by that frame's motion --
// k_undistort's / k_transform_stage's arithmetic: interp_eval + rigid_apply -- and stored.  first <= i < total.
__device__ __forceinline__ int replay_point(const ReplayArgs& a, int t, long long first, long long i, float4& p)
{
  const long long* __restrict__ off = a.off[t];
  int lo = 0, hi = a.nframes - 1;  // the largest f with off[f] <= first (off[0] = 0): its frame is not empty
  while (lo < hi)
  {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= first) lo = mid;
    else hi = mid - 1;
  }
  int f = lo;
  while (off[f + 1] <= i) ++f;  // off[nframes] = total > i
  const float4* __restrict__ src = a.src[t][f];
  const size_t j = (size_t)(i - off[f]);
  p = src[2 * j];
  const float4 q = src[2 * j + 1];
  const FrameMotion& m = a.motion[f];
  Rigid T;
  if (m.interp) interp_eval(m.c, point_time(q), T);
  else T = m.R;
  double ox, oy, oz;
  rigid_apply(T, (double)p.x, (double)p.y, (double)p.z, ox, oy, oz);
  p.x = (float)ox; p.y = (float)oy; p.z = (float)oz;
  a.out[t][2 * (size_t)i] = p;
  a.out[t][2 * (size_t)i + 1] = q;
  return f;
}
// ONE launch for all frames and types (blockIdx.y = type), a thread per logged point.
__global__ __launch_bounds__(256) void k_log_replay(ReplayArgs a, unsigned* __restrict__ bits)
{
  const int t = blockIdx.y;
  const long long total = a.total[t];
  const long long first = (long long)blockIdx.x * 256 + (threadIdx.x & ~63u);  // of this wavefront
  if (first >= total) return;
  const long long i = first + (threadIdx.x & 63u);
  BoxU box;
  bool in_last = false;
  if (i < total)
  {
    float4 p;
    in_last = replay_point(a, t, first, i, p) == a.nframes - 1;
    if (in_last) box_take(box, p.x, p.y, p.z);
  }
  // the last frame's box (pcl::getMinMax3D of keypoints[k] after the loop, Slam.cxx:472-473): only its wavefronts reduce
  if (!__any(in_last)) return;
  box_wave_send(box, bits + 6 * t);
}

// The replay of a RANGE of frames (lsa_kplog_replay_range): the tables hold the range's frames only, the point's arithmetic
// is k_log_replay's, and the box is that of ALL the points of a type (what a sub-map made of the range is rolled onto), not
// of the last frame's: six atomics a workgroup.
__global__ __launch_bounds__(256) void k_log_replay_range(ReplayArgs a, unsigned* __restrict__ bits)
{
  __shared__ unsigned s_box[4][6];
  const int t = blockIdx.y;
  const long long total = a.total[t];
  if ((long long)blockIdx.x * 256 >= total) return;  // (the whole workgroup: nobody is left waiting at the barrier)
  const long long first = (long long)blockIdx.x * 256 + (threadIdx.x & ~63u);  // of this wavefront
  const long long i = first + (threadIdx.x & 63u);
  BoxU box;
  if (i < total)
  {
    float4 p;
    replay_point(a, t, first, i, p);
    box_take(box, p.x, p.y, p.z);
  }
  box_block_send<4>(box, bits + 6 * t, s_box);
}

KpLog* log_of(lsa_ctx* ctx, bool create)
{
  if (!ctx->kplog && create) ctx->kplog = new KpLog;
  return ctx->kplog;
}

// room for `need` bytes in one chunk: the one being filled, one of the free list, or a new one
int reserve(lsa_ctx* ctx, KpLog* log, size_t need, char** at, int* chunk)
{
  if (log->cur >= 0)
  {
    KpLogChunk& c = log->chunks[log->cur];
    if (c.used + need <= c.bytes)
    {
      *at = c.base + c.used;
      *chunk = log->cur;
      c.used += need;
      return LSA_OK;
    }
    if (c.live == 0)  // (filled and emptied again, and too small for this frame)
    {
      c.used = 0;
      log->free_list.push_back(log->cur);
    }
    log->cur = -1;
  }
  for (size_t i = 0; i < log->free_list.size(); ++i)
    if (log->chunks[log->free_list[i]].bytes >= need)
    {
      log->cur = log->free_list[i];
      log->free_list.erase(log->free_list.begin() + (long)i);
      break;
    }
  if (log->cur < 0)
  {
    const size_t bytes = std::max(need, aligned(ctx->kplog_chunk_bytes));
    void* p = nullptr;
    const hipError_t e = ctx->debug_kplog_fail_alloc ? hipErrorOutOfMemory : hipMalloc(&p, bytes);
    if (e != hipSuccess)
    {
      (void)hipGetLastError();
      log->stopped = true;
      return ctx->fail(LSA_E_HIP, std::string("lsa_kplog: a chunk of ") + std::to_string(bytes) + " bytes could not be allocated (" + hipGetErrorString(e) +
                                    "): keypoint logging stops until the log is cleared");
    }
    int slot = -1;
    for (size_t i = 0; i < log->chunks.size() && slot < 0; ++i)
      if (!log->chunks[i].base) slot = (int)i;
    if (slot < 0) { log->chunks.emplace_back(); slot = (int)log->chunks.size() - 1; }
    log->chunks[slot] = KpLogChunk{static_cast<char*>(p), bytes, 0, 0};
    log->held += bytes;
    log->cur = slot;
  }
  KpLogChunk& c = log->chunks[log->cur];
  c.used = need;
  *at = c.base;
  *chunk = log->cur;
  return LSA_OK;
}

int new_frame(lsa_ctx* ctx, KpLog* log, const int n[3], KpLogFrame* out)
{
  KpLogFrame fr;
  size_t need = 0;
  for (int k = 0; k < 3; ++k) need += aligned((size_t)std::max(n[k], 0) * sizeof(lsa_point_t));
  if (need > 0)
  {
    char* at = nullptr;
    const int rc = reserve(ctx, log, need, &at, &fr.chunk);
    if (rc) return rc;
    log->chunks[fr.chunk].live++;
    for (int k = 0; k < 3; ++k)
    {
      fr.n[k] = std::max(n[k], 0);
      if (fr.n[k] > 0) fr.pts[k] = reinterpret_cast<lsa_point_t*>(at);
      at += aligned((size_t)fr.n[k] * sizeof(lsa_point_t));
    }
  }
  *out = fr;
  return LSA_OK;
}

void release_frame(lsa_ctx* ctx, KpLog* log, const KpLogFrame& fr)
{
  if (fr.chunk < 0) return;
  KpLogChunk& c = log->chunks[fr.chunk];
  if (--c.live > 0) return;
  // (what still reads the frame was enqueued on the context's stream before whatever writes the chunk next)
  c.used = 0;
  if (fr.chunk == log->cur) return;
  if (c.bytes == aligned(ctx->kplog_chunk_bytes)) log->free_list.push_back(fr.chunk);
  else
  {
    retire_dev(ctx, c.base);  // a chunk made for one oversized frame
    log->held -= c.bytes;
    c = KpLogChunk{};
  }
}

struct Replay
{
  ReplayArgs args;
  long long total[3];
  int last_n[3];
};

// the per-frame tables: built on the host, uploaded as one block
int prepare_replay(lsa_ctx* ctx, KpLog* log, unsigned type_mask, const double* poses, const double* times, int n, int undistort, Replay* r)
{
  const size_t nf = (size_t)n;
  const size_t motion_bytes = aligned(nf * sizeof(FrameMotion));
  const size_t off_bytes = aligned((nf + 1) * sizeof(long long));
  const size_t src_bytes = aligned(nf * sizeof(const float4*));
  const size_t bytes = motion_bytes + 3 * (off_bytes + src_bytes);
  std::vector<char> host(bytes, 0);
  FrameMotion* motion = reinterpret_cast<FrameMotion*>(host.data());
  for (int i = 0; i < n; ++i)
  {
    FrameMotion& m = motion[i];
    m.interp = (undistort && i >= 1) ? 1 : 0;
    // interpolator.SetTransforms(pose[i - 1], pose[i]); interpolator.SetTimes(t[i] - t[i - 1], 0.)  (Slam.cxx:430-431)
    if (m.interp) m.c = make_interp_const(poses + 16 * (size_t)(i - 1), poses + 16 * (size_t)i, times[i] - times[i - 1], 0.);
    row_major_to_rt(poses + 16 * (size_t)i, m.R.R, m.R.t);
  }
  if (bytes > log->table_cap)
  {
    retire_dev(ctx, log->table);
    log->table = nullptr;
    log->table_cap = 0;
    LSA_HIP(ctx, hipMalloc(&log->table, bytes + bytes / 2));
    log->table_cap = bytes + bytes / 2;
  }
  if (!log->box_dev) LSA_HIP(ctx, hipMalloc((void**)&log->box_dev, 18 * sizeof(unsigned)));
  char* dev = static_cast<char*>(log->table);
  r->args.motion = reinterpret_cast<const FrameMotion*>(dev);
  r->args.nframes = n;
  for (int k = 0; k < 3; ++k)
  {
    const size_t at_off = motion_bytes + (size_t)k * (off_bytes + src_bytes), at_src = at_off + off_bytes;
    long long* off = reinterpret_cast<long long*>(host.data() + at_off);
    const float4** src = reinterpret_cast<const float4**>(host.data() + at_src);
    const bool used = (type_mask >> k) & 1u;
    long long sum = 0;
    for (int i = 0; i < n; ++i)
    {
      off[i] = sum;
      src[i] = reinterpret_cast<const float4*>(log->frames[i].pts[k]);
      if (used) sum += log->frames[i].n[k];
    }
    off[n] = sum;
    r->total[k] = r->args.total[k] = sum;
    r->last_n[k] = used ? log->frames[n - 1].n[k] : 0;
    r->args.off[k] = reinterpret_cast<const long long*>(dev + at_off);
    r->args.src[k] = reinterpret_cast<const float4* const*>(dev + at_src);
    r->args.out[k] = nullptr;
  }
  LSA_HIP(ctx, hipMemcpyAsync(log->table, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `host` goes away
  return LSA_OK;
}

int check_replay(lsa_ctx* ctx, const char* who, unsigned type_mask, const double* poses, const double* times, int n, float last_min[3][3], float last_max[3][3])
{
  if (!ctx) return LSA_E_ARG;
  if (!poses || !times || !last_min || !last_max || (type_mask & ~7u)) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  KpLog* log = ctx->kplog;
  if (log && log->stopped) return ctx->fail(LSA_E_STATE, std::string(who) + ": keypoint logging stopped when a chunk could not be allocated");
  const int have = log ? (int)log->frames.size() : 0;
  if (n != have) return ctx->fail(LSA_E_ARG, std::string(who) + ": " + std::to_string(n) + " poses for " + std::to_string(have) + " logged frames");
  if (n < 2) return ctx->fail(LSA_E_ARG, std::string(who) + ": at least two poses");
  return LSA_OK;
}

// launches the replay (the outputs are set) and reads the last frame's boxes back; waits for the context's stream
int run_replay(lsa_ctx* ctx, KpLog* log, Replay* r, float last_min[3][3], float last_max[3][3])
{
  long long nmax = 0, all = 0;
  for (int k = 0; k < 3; ++k) { nmax = std::max(nmax, r->total[k]); all += r->total[k]; }
  for (int k = 0; k < 3; ++k)
    for (int d = 0; d < 3; ++d) { last_min[k][d] = FLT_MAX; last_max[k][d] = -FLT_MAX; }  // an empty cloud's getMinMax3D
  if (nmax <= 0) return LSA_OK;
  if ((nmax + 255) / 256 > 0x7fffffffLL) return ctx->fail(LSA_E_CAPACITY, "lsa_kplog_replay: more points than one launch addresses");
  unsigned box[18];
  {
    ProfScope ps(ctx, "log_replay", (double)all * 64 + (double)r->args.nframes * (sizeof(FrameMotion) + 3 * 16));
    hipLaunchKernelGGL(k_box_arm, dim3(1), dim3(64), 0, ctx->stream, log->box_dev);
    hipLaunchKernelGGL(k_log_replay, dim3((unsigned)((nmax + 255) / 256), 3), dim3(256), 0, ctx->stream, r->args, log->box_dev);
  }
  LSA_HIP(ctx, hipMemcpyAsync(box, log->box_dev, sizeof(box), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 3; ++k)
    if (r->last_n[k] > 0)
      for (int d = 0; d < 3; ++d)
      {
        // (every coordinate NaN: the words are as they were armed, and so are FLT_MAX / -FLT_MAX)
        if (box[6 * k + d] != kBoxLoArmed) last_min[k][d] = ou2f(box[6 * k + d]);
        if (box[6 * k + 3 + d] != kBoxHiArmed) last_max[k][d] = ou2f(box[6 * k + 3 + d]);
      }
  return LSA_OK;
}
// ---- the replay of a range of frames (lsa_kplog_replay_range and the library's own destinations, lsa_kplog_io.h) ----
int check_range(lsa_ctx* ctx, const char* who, const KpLogRange& q, float box_min[3][3], float box_max[3][3])
{
  if (!ctx) return LSA_E_ARG;
  if (!q.poses || !q.times || !box_min || !box_max || (q.type_mask & ~7u) || q.rule < 0 || q.rule > 2) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  KpLog* log = ctx->kplog;
  if (log && log->stopped) return ctx->fail(LSA_E_STATE, std::string(who) + ": keypoint logging stopped when a chunk could not be allocated");
  const int have = log ? (int)log->frames.size() : 0;
  if (q.n != have) return ctx->fail(LSA_E_ARG, std::string(who) + ": " + std::to_string(q.n) + " poses for " + std::to_string(have) + " logged frames");
  if (q.first < 0 || q.last < q.first || q.last >= q.n)
    return ctx->fail(LSA_E_ARG, std::string(who) + ": frames " + std::to_string(q.first) + ".." + std::to_string(q.last) + " of " + std::to_string(q.n) + " logged ones");
  return LSA_OK;
}

// the tables of the range's frames alone (entry f is frame first + f): what a range costs is what its frames cost
int prepare_range(lsa_ctx* ctx, KpLog* log, const KpLogRange& q, Replay* r)
{
  const int n = q.last - q.first + 1;
  const size_t nf = (size_t)n;
  const size_t motion_bytes = aligned(nf * sizeof(FrameMotion));
  const size_t off_bytes = aligned((nf + 1) * sizeof(long long));
  const size_t src_bytes = aligned(nf * sizeof(const float4*));
  const size_t bytes = motion_bytes + 3 * (off_bytes + src_bytes);
  std::vector<char> host(bytes, 0);
  FrameMotion* motion = reinterpret_cast<FrameMotion*>(host.data());
  for (int f = 0; f < n; ++f)
  {
    const size_t i = (size_t)(q.first + f);
    FrameMotion& m = motion[f];
    m.interp = (q.rule != 0 && i >= 1) ? 1 : 0;
    if (m.interp)
    {
      // rule 1: SetTimes(t[i] - t[i - 1], 0.), the rebuild's (Slam.cxx:431); rule 2: pose[i - 1] one sweep BEFORE pose[i]
      const double dt = q.times[i] - q.times[i - 1];
      m.c = make_interp_const(q.poses + 16 * (i - 1), q.poses + 16 * i, q.rule == 1 ? dt : -dt, 0.);
    }
    row_major_to_rt(q.poses + 16 * i, m.R.R, m.R.t);
  }
  if (bytes > log->table_cap)
  {
    retire_dev(ctx, log->table);
    log->table = nullptr;
    log->table_cap = 0;
    LSA_HIP(ctx, hipMalloc(&log->table, bytes + bytes / 2));
    log->table_cap = bytes + bytes / 2;
  }
  if (!log->box_dev) LSA_HIP(ctx, hipMalloc((void**)&log->box_dev, 18 * sizeof(unsigned)));
  char* dev = static_cast<char*>(log->table);
  r->args.motion = reinterpret_cast<const FrameMotion*>(dev);
  r->args.nframes = n;
  for (int k = 0; k < 3; ++k)
  {
    const size_t at_off = motion_bytes + (size_t)k * (off_bytes + src_bytes), at_src = at_off + off_bytes;
    long long* off = reinterpret_cast<long long*>(host.data() + at_off);
    const float4** src = reinterpret_cast<const float4**>(host.data() + at_src);
    const bool used = (q.type_mask >> k) & 1u;
    long long sum = 0;
    for (int f = 0; f < n; ++f)
    {
      const KpLogFrame& fr = log->frames[(size_t)(q.first + f)];
      off[f] = sum;
      src[f] = reinterpret_cast<const float4*>(fr.pts[k]);
      if (used) sum += fr.n[k];
    }
    off[n] = sum;
    r->total[k] = r->args.total[k] = sum;
    r->last_n[k] = 0;
    r->args.off[k] = reinterpret_cast<const long long*>(dev + at_off);
    r->args.src[k] = reinterpret_cast<const float4* const*>(dev + at_src);
    r->args.out[k] = nullptr;
  }
  LSA_HIP(ctx, hipMemcpyAsync(log->table, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `host` goes away
  return LSA_OK;
}

// launches the range's replay (the outputs are set) and reads the boxes of all its points back; waits for the context's stream
int run_range(lsa_ctx* ctx, KpLog* log, Replay* r, float box_min[3][3], float box_max[3][3])
{
  long long nmax = 0, all = 0;
  for (int k = 0; k < 3; ++k) { nmax = std::max(nmax, r->total[k]); all += r->total[k]; }
  for (int k = 0; k < 3; ++k)
    for (int d = 0; d < 3; ++d) { box_min[k][d] = FLT_MAX; box_max[k][d] = -FLT_MAX; }
  if (nmax <= 0) return LSA_OK;
  if ((nmax + 255) / 256 > 0x7fffffffLL) return ctx->fail(LSA_E_CAPACITY, "lsa_kplog_replay_range: more points than one launch addresses");
  unsigned box[18];
  {
    ProfScope ps(ctx, "log_replay_range", (double)all * 64 + (double)r->args.nframes * (sizeof(FrameMotion) + 3 * 16));
    hipLaunchKernelGGL(k_box_arm, dim3(1), dim3(64), 0, ctx->stream, log->box_dev);
    hipLaunchKernelGGL(k_log_replay_range, dim3((unsigned)((nmax + 255) / 256), 3), dim3(256), 0, ctx->stream, r->args, log->box_dev);
  }
  LSA_HIP(ctx, hipGetLastError());  // (a launch that failed: the outputs may feed another context, which would read them unwritten)
  LSA_HIP(ctx, hipMemcpyAsync(box, log->box_dev, sizeof(box), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < 3; ++k)
    for (int d = 0; d < 3; ++d)
    {
      // (a word as it was armed: no point of the type, or that coordinate NaN in all of them)
      if (box[6 * k + d] != kBoxLoArmed) box_min[k][d] = ou2f(box[6 * k + d]);
      if (box[6 * k + 3 + d] != kBoxHiArmed) box_max[k][d] = ou2f(box[6 * k + 3 + d]);
    }
  return LSA_OK;
}
}  // namespace

namespace lsa
{
// The range straight into a keypoint set of `dst`, a context on the same device (the log's own or another one): nothing of
// the set's survives, the types outside the mask come out empty.  Waits for the stream of the log's context, so whatever
// `dst` enqueues afterwards on its own streams finds the points written.
int kplog_replay_range_to_set(lsa_ctx* ctx, const KpLogRange& q, lsa_ctx* dst, int set, long long counts[3], float box_min[3][3], float box_max[3][3])
{
  const char* who = "lsa_kplog_replay_range (to a keypoint set)";
  int rc = check_range(ctx, who, q, box_min, box_max);
  if (rc) return rc;
  if (!dst || dst->device != ctx->device || set < 0 || set > 2) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  KpLog* log = ctx->kplog;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  Replay r;
  rc = prepare_range(ctx, log, q, &r);
  if (rc) return rc;
  long long nmax = 0;
  for (int k = 0; k < 3; ++k) nmax = std::max(nmax, r.total[k]);
  if (nmax > 0x7fffffffLL - (0x7fffffffLL >> 3)) return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": more points than a keypoint set holds");
  rc = ensure_capacity(dst, (int)nmax);  // (grows the set; waits for the destination's streams when it does)
  if (rc) return dst == ctx ? rc : ctx->fail(rc, std::string(who) + ": " + dst->error);
  LSA_HIP(ctx, hipStreamSynchronize(dst->stream));  // nothing in flight still reads the set
  for (int k = 0; k < 3; ++k) r.args.out[k] = reinterpret_cast<float4*>(dst->kp[set][k]);
  rc = run_range(ctx, log, &r, box_min, box_max);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
  {
    dst->kp_n[set][k] = (int)r.total[k];
    dst->kp_ver[set][k] = ++dst->kp_clock;
    if (counts) counts[k] = r.total[k];
  }
  dst->kp_time_valid[set] = false;
  return LSA_OK;
}

// ... and into the batch buffers of device grids (of one context on the same device, the log's own or another one), followed by
// ONE RollingGrid::Add(range, fixed, time, roll) on each: lsa_kplog_replay_to_grids for a range.
int kplog_replay_range_to_grids(lsa_ctx* ctx, const KpLogRange& q, lsa_device_grid* const grids[3], bool fixed, double time, bool roll, long long counts[3],
                                float box_min[3][3], float box_max[3][3])
{
  const char* who = "lsa_kplog_replay_range (to device grids)";
  int rc = check_range(ctx, who, q, box_min, box_max);
  if (rc) return rc;
  if (!grids) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  for (int k = 0; k < 3; ++k)
    if (((q.type_mask >> k) & 1u) && (!grids[k] || grid_context(grids[k])->device != ctx->device)) return ctx->fail(LSA_E_ARG, std::string(who) + ": a map on this device for every type asked for");
  KpLog* log = ctx->kplog;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  Replay r;
  rc = prepare_range(ctx, log, q, &r);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
  {
    if (counts) counts[k] = r.total[k];
    if (r.total[k] <= 0) continue;
    if (r.total[k] > 0x7fffffffLL) return ctx->fail(LSA_E_CAPACITY, std::string(who) + ": more points than one insertion takes");
    LSA_HIP(ctx, hipStreamSynchronize(grid_stream(grids[k])));  // nothing in flight uses the batch buffer
    lsa_point_t* batch = nullptr;
    rc = grid_batch(grids[k], (int)r.total[k], &batch);
    if (rc) return grid_context(grids[k]) == ctx ? rc : ctx->fail(rc, std::string(who) + ": " + grid_context(grids[k])->error);
    r.args.out[k] = reinterpret_cast<float4*>(batch);
  }
  rc = run_range(ctx, log, &r, box_min, box_max);  // (waits for the context's stream: the batches are written)
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
    if (r.total[k] > 0)
    {
      rc = grid_add_batch(grids[k], (int)r.total[k], fixed, time, roll);
      if (rc) return grid_context(grids[k]) == ctx ? rc : ctx->fail(rc, std::string(who) + ": " + grid_context(grids[k])->error);
    }
  return LSA_OK;
}
}  // namespace lsa

extern "C" {

int lsa_kplog_append(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  KpLog* log = log_of(ctx, true);
  if (log->stopped) return ctx->fail(LSA_E_STATE, "lsa_kplog_append: keypoint logging stopped when a chunk could not be allocated");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  KpLogFrame fr;
  int rc = new_frame(ctx, log, ctx->kp_n[LSA_SET_RAW_CURRENT], &fr);
  if (rc) return rc;
  AppendArgs a;
  int nmax = 0;
  for (int k = 0; k < 3; ++k)
  {
    a.in[k] = reinterpret_cast<const float4*>(ctx->kp[LSA_SET_RAW_CURRENT][k]);
    a.out[k] = reinterpret_cast<float4*>(fr.pts[k]);
    a.n[k] = fr.n[k];
    nmax = std::max(nmax, fr.n[k]);
  }
  // one launch on the registration stream, behind whatever wrote the keypoints: they never visit the host
  if (nmax > 0) hipLaunchKernelGGL(k_log_append, dim3((nmax + 255) / 256, 3), dim3(256), 0, ctx->stream, a);
  log->frames.push_back(fr);
  return LSA_OK;
}

int lsa_kplog_append_points(lsa_ctx* ctx, const lsa_point_t* const pts[3], const int n[3])
{
  if (!ctx) return LSA_E_ARG;
  if (!pts || !n) return ctx->fail(LSA_E_ARG, "lsa_kplog_append_points: bad argument");
  for (int k = 0; k < 3; ++k)
    if (n[k] < 0 || (n[k] > 0 && !pts[k])) return ctx->fail(LSA_E_ARG, "lsa_kplog_append_points: bad argument");
  KpLog* log = log_of(ctx, true);
  if (log->stopped) return ctx->fail(LSA_E_STATE, "lsa_kplog_append_points: keypoint logging stopped when a chunk could not be allocated");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  KpLogFrame fr;
  int rc = new_frame(ctx, log, n, &fr);
  if (rc) return rc;
  log->frames.push_back(fr);
  bool any = false;
  for (int k = 0; k < 3; ++k)
    if (fr.n[k] > 0)
    {
      LSA_HIP(ctx, hipMemcpyAsync(fr.pts[k], pts[k], (size_t)fr.n[k] * sizeof(lsa_point_t), hipMemcpyHostToDevice, ctx->stream));
      any = true;
    }
  if (any) LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // pts may be pageable and reused by the caller
  return LSA_OK;
}

int lsa_kplog_pop_front(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  KpLog* log = ctx->kplog;
  if (!log || log->frames.empty()) return ctx->fail(LSA_E_STATE, "lsa_kplog_pop_front: the log is empty");
  const KpLogFrame fr = log->frames.front();
  log->frames.pop_front();
  release_frame(ctx, log, fr);
  place_pop_front(ctx);
  return LSA_OK;
}

int lsa_kplog_clear(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  KpLog* log = ctx->kplog;
  if (!log) return LSA_OK;
  // the chunks go to the graveyard: freed at the start of the next frame, when nothing in flight can still read them
  for (KpLogChunk& c : log->chunks)
    if (c.base) retire_dev(ctx, c.base);
  log->chunks.clear();
  log->free_list.clear();
  log->frames.clear();
  log->cur = -1;
  log->held = 0;
  log->stopped = false;
  place_clear(ctx);
  return LSA_OK;
}

int lsa_kplog_size(const lsa_ctx* ctx) { return ctx && ctx->kplog ? (int)ctx->kplog->frames.size() : 0; }

int lsa_kplog_count(const lsa_ctx* ctx, int frame, int type)
{
  if (!ctx || type < 0 || type > 2) return LSA_E_ARG;
  const KpLog* log = ctx->kplog;
  if (!log || frame < 0 || frame >= (int)log->frames.size()) return LSA_E_ARG;
  return log->frames[frame].n[type];
}

int lsa_kplog_get(lsa_ctx* ctx, int frame, int type, lsa_point_t* out, int capacity)
{
  if (!ctx) return LSA_E_ARG;
  KpLog* log = ctx->kplog;
  if (type < 0 || type > 2 || capacity < 0 || (!out && capacity > 0) || !log || frame < 0 || frame >= (int)log->frames.size())
    return ctx->fail(LSA_E_ARG, "lsa_kplog_get: bad argument");
  const KpLogFrame& fr = log->frames[frame];
  const int n = std::min(capacity, fr.n[type]);
  if (n <= 0) return 0;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipMemcpyAsync(out, fr.pts[type], (size_t)n * sizeof(lsa_point_t), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return n;
}

unsigned long long lsa_kplog_bytes(const lsa_ctx* ctx) { return ctx && ctx->kplog ? (unsigned long long)ctx->kplog->held : 0ull; }

int lsa_kplog_stopped(const lsa_ctx* ctx) { return ctx && ctx->kplog && ctx->kplog->stopped ? 1 : 0; }

int lsa_kplog_replay(lsa_ctx* ctx, unsigned type_mask, const double* poses, const double* times, int n, int undistort, lsa_point_t* const out[3],
                     float last_min[3][3], float last_max[3][3])
{
  int rc = check_replay(ctx, "lsa_kplog_replay", type_mask, poses, times, n, last_min, last_max);
  if (rc) return rc;
  KpLog* log = ctx->kplog;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  Replay r;
  rc = prepare_replay(ctx, log, type_mask, poses, times, n, undistort, &r);
  if (rc) return rc;
  // the device writes straight into pinned host memory (what the host maps insert from, lsa_kplog_replayed)
  for (int k = 0; k < 3; ++k)
  {
    log->stage_n[k] = 0;
    if (r.total[k] > log->stage_cap[k])
    {
      retire_host(ctx, log->stage[k]);
      log->stage[k] = nullptr;
      log->stage_cap[k] = 0;
      const long long cap = r.total[k] + r.total[k] / 4;
      LSA_HIP(ctx, hipHostMalloc((void**)&log->stage[k], (size_t)cap * sizeof(lsa_point_t), hipHostMallocDefault));
      log->stage_cap[k] = cap;
    }
    r.args.out[k] = reinterpret_cast<float4*>(log->stage[k]);
  }
  rc = run_replay(ctx, log, &r, last_min, last_max);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
  {
    log->stage_n[k] = r.total[k];
    if (out && out[k] && r.total[k] > 0) std::memcpy(out[k], log->stage[k], (size_t)r.total[k] * sizeof(lsa_point_t));
  }
  return LSA_OK;
}

long long lsa_kplog_replayed(const lsa_ctx* ctx, int type, const lsa_point_t** pts)
{
  if (!ctx || type < 0 || type > 2 || !pts || !ctx->kplog) return LSA_E_ARG;
  *pts = ctx->kplog->stage[type];
  return ctx->kplog->stage_n[type];
}

int lsa_kplog_replay_range(lsa_ctx* ctx, unsigned type_mask, const double* poses, const double* times, int n, int first, int last, int rule, lsa_point_t* const out[3],
                           float box_min[3][3], float box_max[3][3])
{
  const KpLogRange q{type_mask, poses, times, n, first, last, rule};
  int rc = check_range(ctx, "lsa_kplog_replay_range", q, box_min, box_max);
  if (rc) return rc;
  KpLog* log = ctx->kplog;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  Replay r;
  rc = prepare_range(ctx, log, q, &r);
  if (rc) return rc;
  // into the pinned staging of the whole-log replay (lsa_kplog_replayed reads either)
  for (int k = 0; k < 3; ++k)
  {
    log->stage_n[k] = 0;
    if (r.total[k] > log->stage_cap[k])
    {
      retire_host(ctx, log->stage[k]);
      log->stage[k] = nullptr;
      log->stage_cap[k] = 0;
      const long long cap = r.total[k] + r.total[k] / 4;
      LSA_HIP(ctx, hipHostMalloc((void**)&log->stage[k], (size_t)cap * sizeof(lsa_point_t), hipHostMallocDefault));
      log->stage_cap[k] = cap;
    }
    r.args.out[k] = reinterpret_cast<float4*>(log->stage[k]);
  }
  rc = run_range(ctx, log, &r, box_min, box_max);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k)
  {
    log->stage_n[k] = r.total[k];
    if (out && out[k] && r.total[k] > 0) std::memcpy(out[k], log->stage[k], (size_t)r.total[k] * sizeof(lsa_point_t));
  }
  return LSA_OK;
}

int lsa_kplog_replay_to_grids(lsa_ctx* ctx, unsigned type_mask, const double* poses, const double* times, int n, int undistort, lsa_device_grid* const grids[3],
                              float last_min[3][3], float last_max[3][3])
{
  int rc = check_replay(ctx, "lsa_kplog_replay_to_grids", type_mask, poses, times, n, last_min, last_max);
  if (rc) return rc;
  if (!grids) return ctx->fail(LSA_E_ARG, "lsa_kplog_replay_to_grids: bad argument");
  for (int k = 0; k < 3; ++k)
    if (((type_mask >> k) & 1u) && (!grids[k] || grid_context(grids[k]) != ctx)) return ctx->fail(LSA_E_ARG, "lsa_kplog_replay_to_grids: a map of this context for every type asked for");
  KpLog* log = ctx->kplog;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  Replay r;
  rc = prepare_replay(ctx, log, type_mask, poses, times, n, undistort, &r);
  if (rc) return rc;
  // straight into the maps' batch buffers, which the insertion reads: the maps' stream has nothing in flight that uses them
  for (int k = 0; k < 3; ++k)
  {
    if (r.total[k] <= 0) continue;
    if (r.total[k] > 0x7fffffffLL) return ctx->fail(LSA_E_CAPACITY, "lsa_kplog_replay_to_grids: more points than one insertion takes");
    LSA_HIP(ctx, hipStreamSynchronize(grid_stream(grids[k])));
    lsa_point_t* batch = nullptr;
    rc = grid_batch(grids[k], (int)r.total[k], &batch);
    if (rc) return rc;
    r.args.out[k] = reinterpret_cast<float4*>(batch);
  }
  rc = run_replay(ctx, log, &r, last_min, last_max);  // (waits for the context's stream: the batches are written)
  if (rc) return rc;
  // LocalMaps[k]->Add(aggregatedKeypointsMap[k], false, -1., false)  (Slam.cxx:474): one Add that does not roll
  for (int k = 0; k < 3; ++k)
    if (r.total[k] > 0)
    {
      rc = grid_add_batch(grids[k], (int)r.total[k], false, -1., false);
      if (rc) return rc;
    }
  return LSA_OK;
}

}  // extern "C"
