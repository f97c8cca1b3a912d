// lsa_upload.hip -- a LidarPoint cloud on its way to the device: the plain upload, the inbox of frames uploaded ahead with
// its uploader threads, the frame store, the host-side azimuthal resolution estimate.
#include <algorithm>
#include <cmath>
#include "lsa_ctx.h"

using namespace lsa;

namespace lsa
{

// SpinningSensorKeypointExtractor::EstimateAzimuthalResolution (SSKE.cxx:593-637), run on
// the host once, on the first usable frame: its float arithmetic (acos) feeds a threshold of
// the invalidation pass, so it must be the libm the reference itself would use.
static float estimate_azimuthal_resolution(const lsa_point_t* pts, int n)
{
  // last point seen per ring (arrival order inside a ring is the scan order)
  std::vector<int> last(kMaxRings, -1);
  std::vector<std::vector<float>> perRing(kMaxRings);
  for (int i = 0; i < n; ++i)
  {
    unsigned r = pts[i].laser_id;
    if (r >= (unsigned)kMaxRings) continue;
    if (last[r] >= 0)
    {
      const lsa_point_t& a = pts[last[r]];
      const lsa_point_t& b = pts[i];
      float d = a.x * b.x + a.y * b.y;
      float na = std::sqrt(a.x * a.x + a.y * a.y), nb = std::sqrt(b.x * b.x + b.y * b.y);
      float angle = std::abs(std::acos(d / (na * nb)));
      if (angle > 1e-4) perRing[r].push_back(angle);
    }
    last[r] = i;
  }
  std::vector<float> angles;
  angles.reserve(n);
  for (auto& v : perRing) angles.insert(angles.end(), v.begin(), v.end());
  if (angles.size() < 100) return 0.f;
  std::sort(angles.begin(), angles.end());
  unsigned maxInliersIdx = angles.size();
  float maxAngle = float(5. / 180. * M_PI);
  float medianAngle = 0.f;
  while (maxAngle > 1.8 * medianAngle)
  {
    maxInliersIdx = std::upper_bound(angles.begin(), angles.begin() + maxInliersIdx, maxAngle) - angles.begin();
    medianAngle = angles[maxInliersIdx / 2];
    maxAngle = std::min(medianAngle * 2., maxAngle / 1.8);
  }
  return medianAngle;
}

void maybe_estimate_resolution(lsa_ctx* ctx, const lsa_point_t* pts, int n)
{
  if (ctx->az_res < 1e-6 || M_PI / 4. < ctx->az_res)
  {
    float v = estimate_azimuthal_resolution(pts, n);
    if (v > 0.f) ctx->az_res = v;
  }
}

// FNV-1a over 32 points spread evenly over the cloud (and its size): tells a buffer that was rewritten in place from the
// one that was announced.  Every sample is a cache miss in the caller's 8 MB on the frame's critical path (AddFrame
// compares before it takes the upload over): 256 samples cost 25 us a frame, 32 cost 3 -- and another scan in the same
// buffer differs in practically every point.
static unsigned long long cloud_fingerprint(const lsa_point_t* pts, int n)
{
  unsigned long long h = 1469598103934665603ull ^ (unsigned long long)n;
  const int samples = std::min(n, 32);
  for (int i = 0; i < samples; ++i)
  {
    const size_t at = (size_t)i * (size_t)n / (size_t)samples;
    unsigned long long w[sizeof(lsa_point_t) / 8];
    std::memcpy(w, pts + at, sizeof(w));
    for (unsigned long long v : w) { h ^= v; h *= 1099511628211ull; }
  }
  return h;
}

// piece `part` of the cloud being uploaded: pageable -> pinned staging -> DMA on the copy stream (any thread, any order)
static bool upload_part(lsa_ctx* ctx, const lsa_ctx::UploadSplit& u, int part)
{
  const size_t b = u.points * (size_t)part / (size_t)u.parts * sizeof(lsa_point_t), e = u.points * (size_t)(part + 1) / (size_t)u.parts * sizeof(lsa_point_t);
  if (e <= b) return true;
  std::memcpy(u.pinned + b, u.src + b, e - b);
  return hipMemcpyAsync(u.dev + b, u.pinned + b, e - b, hipMemcpyHostToDevice, ctx->copy_stream) == hipSuccess;
}
static void upload_helper_main(lsa_ctx* ctx, int part)
{
  (void)hipSetDevice(ctx->device);
  unsigned long long seen = 0;
  std::unique_lock<std::mutex> l(ctx->up_mutex);
  while (true)
  {
    ctx->up_help_cv.wait(l, [&] { return ctx->up_quit || ctx->up_split.seq != seen; });
    if (ctx->up_quit) return;
    seen = ctx->up_split.seq;
    const lsa_ctx::UploadSplit u = ctx->up_split;
    l.unlock();
    const bool ok = part < u.parts ? upload_part(ctx, u, part) : true;
    l.lock();
    if (ctx->up_split.seq == seen)  // (a helper that woke up for a cloud nobody split has nothing to report to the next one)
    {
      ctx->up_split.ok = ctx->up_split.ok && ok;
      ctx->up_split.done++;
      ctx->up_help_done.notify_all();
    }
  }
}
// the uploader thread of a context: pageable cloud -> pinned staging -> DMA on the copy stream -> event, in up_parts pieces
// side by side (this thread takes the first, a helper each of the others)
static void uploader_main(lsa_ctx* ctx)
{
  (void)hipSetDevice(ctx->device);
  std::unique_lock<std::mutex> l(ctx->up_mutex);
  while (true)
  {
    ctx->up_cv.wait(l, [ctx] { return ctx->up_quit || !ctx->up_jobs.empty(); });
    if (ctx->up_quit || ctx->up_jobs.empty()) return;  // on the way out the queued clouds are not touched: their owner may have freed them
    const int slot = ctx->up_jobs.front();
    ctx->up_jobs.pop_front();
    FrameInbox& in = ctx->inbox[slot];
    const int helpers = (int)ctx->up_helpers.size();
    lsa_ctx::UploadSplit& u = ctx->up_split;
    u.src = reinterpret_cast<const char*>(in.src); u.pinned = reinterpret_cast<char*>(in.pinned); u.dev = reinterpret_cast<char*>(in.dev);
    u.points = (size_t)in.n;
    u.parts = in.n >= 65536 ? helpers + 1 : 1;  // (a small cloud is not worth waking anybody)
    u.done = 0; u.ok = true;
    u.seq++;
    const lsa_ctx::UploadSplit mine = u;
    if (mine.parts > 1) ctx->up_help_cv.notify_all();
    l.unlock();
    bool ok = upload_part(ctx, mine, 0);
    l.lock();
    if (mine.parts > 1) ctx->up_help_done.wait(l, [&] { return ctx->up_split.done >= helpers || ctx->up_quit; });
    ok = ok && ctx->up_split.ok;
    l.unlock();
    in.fingerprint = cloud_fingerprint(in.pinned, in.n);
    ok = ok && hipEventRecord(in.ev, ctx->copy_stream) == hipSuccess;
    l.lock();
    in.state.store(ok ? 2 : -1, std::memory_order_release);
    ctx->up_done.notify_all();
  }
}

}  // namespace lsa

extern "C" {

// gives up the oldest frame uploaded ahead: its DMA has to be over before its buffers are reused
static int inbox_drop_front(lsa_ctx* ctx)
{
  FrameInbox& old = ctx->inbox[ctx->inbox_queue.front()];
  {
    std::unique_lock<std::mutex> l(ctx->up_mutex);
    ctx->up_done.wait(l, [&] { return old.state.load() != 1; });
  }
  if (old.state.load() == 2) LSA_HIP(ctx, hipEventSynchronize(old.ev));
  if (ctx->prefetch_pending && ctx->prefetch_frame == old.dev)
  {
    LSA_HIP(ctx, hipStreamSynchronize(ctx->prefetch_stream));
    ctx->prefetch_pending = false;
  }
  old.state.store(0);
  ctx->inbox_queue.pop_front();
  return LSA_OK;
}

int lsa_upload_frame_begin(lsa_ctx* ctx, const lsa_point_t* pts, int n)
{
  if (!ctx || !pts || n <= 0) return ctx ? ctx->fail(LSA_E_ARG, "lsa_upload_frame_begin: empty frame") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  // two frames ahead at most: the cloud of the next AddFrame (announced during the previous one) and the one after it
  while (ctx->inbox_queue.size() >= 2)
  {
    const int rc = inbox_drop_front(ctx);
    if (rc) return rc;
  }
  int slot = -1;
  for (int c = 0; c < 3 && slot < 0; ++c)
  {
    bool used = c == ctx->inbox_current;
    for (int q : ctx->inbox_queue) used = used || q == c;
    if (!used) slot = c;
  }
  if (slot < 0) return ctx->fail(LSA_E_STATE, "lsa_upload_frame_begin: no free buffer");
  FrameInbox& in = ctx->inbox[slot];
  if (!ctx->uploader.joinable())
  {
    if (const char* e = std::getenv("LSA_UPLOAD_THREADS")) ctx->up_parts = std::min(std::max(std::atoi(e), 1), 8);
    for (int h = 1; h < ctx->up_parts; ++h) ctx->up_helpers.emplace_back(upload_helper_main, ctx, h);
    ctx->uploader = std::thread(uploader_main, ctx);
  }
  if (!in.ev) LSA_HIP(ctx, hipEventCreateWithFlags(&in.ev, hipEventDisableTiming));
  if (in.cap < n)
  {
    // (this slot's last frame is at least two AddFrame calls old: nothing reads it any more)
    retire_dev(ctx, in.dev);
    retire_host(ctx, in.pinned);
    in.dev = nullptr; in.pinned = nullptr; in.cap = 0;
    const int cap = n + n / 8;
    LSA_HIP(ctx, hipMalloc((void**)&in.dev, (size_t)cap * sizeof(lsa_point_t)));
    LSA_HIP(ctx, hipHostMalloc((void**)&in.pinned, (size_t)cap * sizeof(lsa_point_t), hipHostMallocDefault));
    in.cap = cap;
  }
  in.n = n;
  in.src = pts;
  LSA_HIP(ctx, frame_writer_guard(ctx, ctx->copy_stream));  // this slot's last frame may still be read by the dense map's insertion
  in.state.store(1, std::memory_order_release);
  ctx->inbox_queue.push_back(slot);
  {
    std::lock_guard<std::mutex> l(ctx->up_mutex);
    ctx->up_jobs.push_back(slot);
  }
  ctx->up_cv.notify_one();
  return LSA_OK;
}

int lsa_upload_frame_ready(const lsa_ctx* ctx)
{
  if (!ctx || ctx->inbox_queue.empty()) return 0;
  return ctx->inbox[ctx->inbox_queue.front()].state.load(std::memory_order_acquire) == 2 ? 1 : 0;
}

int lsa_upload_frame_adopt(lsa_ctx* ctx, const lsa_point_t* pts, int n)
{
  if (!ctx) return LSA_E_ARG;
  // the announced cloud this one is, if any (clouds announced before it were skipped by the caller: given up)
  size_t at = ctx->inbox_queue.size();
  for (size_t i = 0; i < ctx->inbox_queue.size() && at == ctx->inbox_queue.size(); ++i)
    if (ctx->inbox[ctx->inbox_queue[i]].src == pts && ctx->inbox[ctx->inbox_queue[i]].n == n) at = i;
  if (at == ctx->inbox_queue.size()) return 0;  // not announced: the caller uploads this one itself
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  for (size_t i = 0; i < at; ++i)
  {
    const int rc = inbox_drop_front(ctx);
    if (rc) return rc;
  }
  const int slot = ctx->inbox_queue.front();
  FrameInbox& in = ctx->inbox[slot];
  {
    std::unique_lock<std::mutex> l(ctx->up_mutex);
    ctx->up_done.wait(l, [&] { return in.state.load() != 1; });
  }
  ctx->inbox_queue.pop_front();
  if (in.state.load() != 2)
  {
    in.state.store(0);
    return ctx->fail(LSA_E_HIP, "lsa_upload_frame_adopt: the upload failed");
  }
  if (in.fingerprint != cloud_fingerprint(pts, n))
  {
    // same address and size, other contents: the buffer was reused for another scan since it was announced (a driver's
    // ring buffer, an allocator handing the same block out again) -- the copy made then is stale, the caller uploads
    LSA_HIP(ctx, hipEventSynchronize(in.ev));
    if (ctx->prefetch_pending && ctx->prefetch_frame == in.dev)
    {
      LSA_HIP(ctx, hipStreamSynchronize(ctx->prefetch_stream));
      ctx->prefetch_pending = false;
    }
    in.state.store(0);
    return 0;
  }
  int rc = ensure_capacity(ctx, n);
  if (rc) return rc;
  maybe_estimate_resolution(ctx, pts, n);
  LSA_HIP(ctx, hipStreamWaitEvent(ctx->stream, in.ev, 0));
  ctx->frame = in.dev;
  ctx->frame_n = n;
  ctx->inbox_current = slot;
  in.state.store(0);
  ctx->uploads_adopted++;
  return 1;
}

int lsa_upload_frame_forget(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  while (!ctx->inbox_queue.empty())
  {
    const int rc = inbox_drop_front(ctx);
    if (rc) return rc;
  }
  return LSA_OK;
}

int lsa_pin_host_memory(void* ptr, size_t bytes)
{
  if (!ptr || bytes == 0) return LSA_E_ARG;
  return hipHostRegister(ptr, bytes, hipHostRegisterPortable) == hipSuccess ? LSA_OK : LSA_E_HIP;
}
int lsa_unpin_host_memory(void* ptr)
{
  if (!ptr) return LSA_E_ARG;
  return hipHostUnregister(ptr) == hipSuccess ? LSA_OK : LSA_E_HIP;
}

int lsa_uploads_adopted(const lsa_ctx* ctx) { return ctx ? ctx->uploads_adopted : 0; }

int lsa_upload_frame(lsa_ctx* ctx, const lsa_point_t* pts, int n)
{
  if (!ctx || !pts || n <= 0) return ctx ? ctx->fail(LSA_E_ARG, "lsa_upload_frame: empty frame") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure_capacity(ctx, n);
  if (rc) return rc;
  maybe_estimate_resolution(ctx, pts, n);
  LSA_HIP(ctx, frame_writer_guard(ctx, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(ctx->frame_own, pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyHostToDevice, ctx->stream));
  ctx->frame = ctx->frame_own;
  ctx->frame_n = n;
  ctx->inbox_current = -1;
  return LSA_OK;
}

int lsa_frame_store_put(lsa_ctx* ctx, int slot, const lsa_point_t* pts, int n)
{
  if (!ctx || !pts || n <= 0 || slot < 0 || slot > 65536) return ctx ? ctx->fail(LSA_E_ARG, "lsa_frame_store_put: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure_capacity(ctx, n);
  if (rc) return rc;
  if ((int)ctx->store.size() <= slot) { ctx->store.resize(slot + 1, {nullptr, 0}); ctx->store_cap.resize(slot + 1, 0); }
  lsa_point_t* d = ctx->store[slot].first;
  if (ctx->prefetch_pending && d && ctx->prefetch_frame == d)
  {
    // the look-ahead extraction reads this slot: let it finish, its result no longer describes the slot
    LSA_HIP(ctx, hipStreamSynchronize(ctx->prefetch_stream));
    ctx->prefetch_pending = false;
  }
  if (!d || ctx->store_cap[slot] < n)
  {
    // the frame in use may be this very slot: nothing may still read it
    LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (d) { if (ctx->frame == d) { ctx->frame = nullptr; ctx->frame_n = 0; } retire_dev(ctx, d); ctx->store[slot] = {nullptr, 0}; ctx->store_cap[slot] = 0; }
    d = nullptr;
    LSA_HIP(ctx, hipMalloc((void**)&d, (size_t)n * sizeof(lsa_point_t)));
    ctx->store_cap[slot] = n;
  }
  LSA_HIP(ctx, frame_writer_guard(ctx, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(d, pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyHostToDevice, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // pts may be pageable and reused by the caller
  ctx->store[slot] = {d, n};
  if (ctx->frame == d) ctx->frame_n = n;
  maybe_estimate_resolution(ctx, pts, n);
  return LSA_OK;
}

int lsa_frame_store_use(lsa_ctx* ctx, int slot)
{
  if (!ctx || slot < 0 || slot >= (int)ctx->store.size() || !ctx->store[slot].first)
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_frame_store_use: empty slot") : LSA_E_ARG;
  LSA_HIP(ctx, frame_writer_guard(ctx, ctx->stream));  // what works on the slot in place next (times from the advancement) comes behind a dense-map insertion that reads it
  ctx->frame = ctx->store[slot].first;
  ctx->frame_n = ctx->store[slot].second;
  ctx->inbox_current = -1;
  return LSA_OK;
}

}  // extern "C"
