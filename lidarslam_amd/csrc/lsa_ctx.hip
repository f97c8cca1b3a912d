// lsa_ctx.hip -- context lifetime, device buffers and their growth, the graveyard of outgrown buffers, the small getters.
#include <algorithm>
#include <cctype>
#include <sched.h>
#include "lsa_ctx.h"

using namespace lsa;

namespace lsa
{

// (re)allocation of a device buffer of the context: what it held is retired, not freed (lsa_ctx.h: grave_dev)
template <typename T> static hipError_t dev_alloc(lsa_ctx* ctx, T** p, size_t count)
{
  if (*p) { retire_dev(ctx, *p); *p = nullptr; }
  return hipMalloc((void**)p, std::max<size_t>(count, 1) * sizeof(T));
}

int ensure_capacity(lsa_ctx* ctx, int n)
{
  if (n <= ctx->cap_n) return LSA_OK;
  // grow geometrically so that a sequence with slightly varying scan sizes allocates once
  int cap = std::max(n + n / 8, 4096);
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // a look-ahead extraction in flight writes into buffers that are about to move: let it finish and forget it
  if (ctx->prefetch_stream) LSA_HIP(ctx, hipStreamSynchronize(ctx->prefetch_stream));
  ctx->prefetch_pending = false;
  for (int k = 0; k < 3; ++k) LSA_HIP(ctx, dev_alloc(ctx, &ctx->kp_next[k], (size_t)cap));
  // keypoint sets must survive a growth (raw previous is still needed): copy them over -- on the context's stream and waited
  // for below.  (A device-to-device hipMemcpy goes to the null stream, which the context's non-blocking streams are not ordered
  // with, and need not block the host: the old frame could land in the new buffer AFTER the upload that follows the growth
  // and overwrite its head -- the first frame of a larger scan then came out with the points of the frame before in front.)
  bool carried = false;
  lsa_point_t* old_kp[3][3];
  for (int s = 0; s < 3; ++s)
    for (int k = 0; k < 3; ++k) { old_kp[s][k] = ctx->kp[s][k]; ctx->kp[s][k] = nullptr; }
  for (int s = 0; s < 3; ++s)
    for (int k = 0; k < 3; ++k)
    {
      LSA_HIP(ctx, dev_alloc(ctx, &ctx->kp[s][k], (size_t)cap));
      if (old_kp[s][k] && ctx->kp_n[s][k] > 0)
      {
        LSA_HIP(ctx, hipMemcpyAsync(ctx->kp[s][k], old_kp[s][k], (size_t)ctx->kp_n[s][k] * sizeof(lsa_point_t), hipMemcpyDeviceToDevice, ctx->stream));
        carried = true;
      }
      retire_dev(ctx, old_kp[s][k]);
    }
  {
    // an uploaded frame must survive too (a further device frame may need more room for the merged keypoints)
    lsa_point_t* old_frame = ctx->frame_own;
    const bool current = old_frame && ctx->frame == old_frame && ctx->frame_n > 0;
    ctx->frame_own = nullptr;
    LSA_HIP(ctx, dev_alloc(ctx, &ctx->frame_own, (size_t)cap));
    if (current)
    {
      LSA_HIP(ctx, hipMemcpyAsync(ctx->frame_own, old_frame, (size_t)ctx->frame_n * sizeof(lsa_point_t), hipMemcpyDeviceToDevice, ctx->stream));
      carried = true;
      ctx->frame = ctx->frame_own;
    }
    retire_dev(ctx, old_frame);
  }
  LSA_HIP(ctx, dev_alloc(ctx, &ctx->xyzi, (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &ctx->orig, (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &ctx->ring_of, (size_t)cap));
  int nblocks = (cap + kBucketChunk - 1) / kBucketChunk;
  LSA_HIP(ctx, dev_alloc(ctx, &ctx->block_hist, (size_t)nblocks * kMaxRings));
  for (int i = 0; i < 4; ++i) LSA_HIP(ctx, dev_alloc(ctx, &ctx->score[i], (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &ctx->valid, (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &ctx->label, (size_t)cap));
  ctx->cap_n = cap;
  if (carried) LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // every stream of the context may use the new buffers from here on
  return LSA_OK;
}

int ensure_target(lsa_ctx* ctx, int ti, int m)
{
  Target& t = ctx->target[ti];
  if (!t.desc)
  {
    for (int l = 0; l < kGridLevels; ++l)
    {
      GridLevel& g = t.lv[l];
      g.max_cells = grid_level_cells(l);
      LSA_HIP(ctx, dev_alloc(ctx, &g.cell_start, (size_t)g.max_cells + 1));
      LSA_HIP(ctx, dev_alloc(ctx, &g.cell_fill, (size_t)g.max_cells));
      LSA_HIP(ctx, dev_alloc(ctx, &g.block_sums, (size_t)g.max_cells / 1024 + 2));
    }
    LSA_HIP(ctx, dev_alloc(ctx, &t.desc, kGridLevels));
    LSA_HIP(ctx, dev_alloc(ctx, &t.bbox_bits, 8));
    // armed once here, re-armed by k_grid_scatter after every build
    const int init[8] = {0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000, 0, 0};
    LSA_HIP(ctx, hipMemcpy(t.bbox_bits, init, sizeof(init), hipMemcpyHostToDevice));
  }
  if (m <= t.cap) return LSA_OK;
  // doubling from 64 k points (7 MB a target): a growing sub-map re-allocates a handful of times in a sequence's life -- each
  // time eight buffers are retired and freed at the next frame's start, where every hipFree waits for the device (0.3-0.6 ms:
  // with a floor of 16 k a map's first hundred keyframes crossed it for every target, 15 us a frame over bench.py's window)
  int cap = std::max(2 * m, 65536);
  // (no synchronisation: the outgrown buffers are retired, launches in flight keep them; the new ones are filled before
  // they are read.  This runs on worker threads too, beside ICP iterations enqueued ahead)
  LSA_HIP(ctx, dev_alloc(ctx, &t.pts, (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &t.xyzl, (size_t)cap));
  for (int l = 0; l < kGridLevels; ++l)
  {
    LSA_HIP(ctx, dev_alloc(ctx, &t.lv[l].sorted, (size_t)cap));
    LSA_HIP(ctx, dev_alloc(ctx, &t.lv[l].cell_of, (size_t)cap));
  }
  t.cap = cap;
  return LSA_OK;
}

int ensure_match(lsa_ctx* ctx, int type, int k)
{
  MatchBuf& b = ctx->match[type];
  if (k <= b.cap) return LSA_OK;
  int cap = std::max(k + k / 4, 4096);
  LSA_HIP(ctx, dev_alloc(ctx, &b.rec, (size_t)cap * 16));
  LSA_HIP(ctx, dev_alloc(ctx, &b.status, (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &b.knn_idx, (size_t)cap * kKnnMax));
  LSA_HIP(ctx, dev_alloc(ctx, &b.knn_d2, (size_t)cap * kKnnMax));
  LSA_HIP(ctx, dev_alloc(ctx, &b.knn_cnt, (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &b.slow_list, (size_t)cap));
  LSA_HIP(ctx, dev_alloc(ctx, &b.slow_pts, (size_t)cap));
  b.cap = cap;
  b.knn_n = 0;  // the lists stayed in the outgrown buffers
  return LSA_OK;
}

int ensure_scratch(lsa_ctx* ctx, size_t bytes)
{
  if (bytes <= ctx->scratch_cap) return LSA_OK;
  retire_dev(ctx, ctx->scratch_out);
  ctx->scratch_out = nullptr;
  LSA_HIP(ctx, hipMalloc(&ctx->scratch_out, bytes + bytes / 4));
  ctx->scratch_cap = bytes + bytes / 4;
  return LSA_OK;
}

}  // namespace lsa

extern "C" {

int lsa_collect_garbage(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  std::vector<void*> dev, host;
  {
    std::lock_guard<std::mutex> l(ctx->grave_mutex);
    dev.swap(ctx->grave_dev);
    host.swap(ctx->grave_host);
  }
  if (dev.empty() && host.empty()) return LSA_OK;
  if (std::getenv("LSA_STAGE_DEBUG")) std::fprintf(stderr, "[garbage debug] %zu device and %zu host buffers freed\n", dev.size(), host.size());
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  for (void* p : dev) (void)hipFree(p);       // (waits for the device: every launch that could still read them is over)
  for (void* p : host) (void)hipHostFree(p);
  return LSA_OK;
}

int lsa_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int lsa_ctx_create(int device_id, lsa_ctx** out)
{
  if (!out) return LSA_E_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n)
    return LSA_E_NO_DEVICE;  // no CPU fallback: the caller must fail loudly
  if (hipSetDevice(device_id) != hipSuccess) return LSA_E_HIP;
  lsa_ctx* ctx = new lsa_ctx;
  ctx->device = device_id;
  g_live_contexts.fetch_add(1, std::memory_order_relaxed);
  // EXACTLY THREE streams per context, created together: the registration's, the look-ahead's, the copies'.  The runtime
  // deals streams to the process's four hardware queues in creation order (GPU_MAX_HW_QUEUES = 4, round robin), and two
  // streams on one queue wait for each other's kernels.  Three in a row sit on three different queues, and the next
  // context's three start one queue further: with four streams per context every context's registration stream landed
  // on the same queue (8 sequences side by side: 1 200 frames/s against 2 000), and any further stream of a context
  // shares the registration's queue (a stream for the maps: 765 against 890 frames/s for one sequence).  The side streams
  // of the staged (non-fused) match are created when that path is first used.
  if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { g_live_contexts.fetch_sub(1, std::memory_order_relaxed); delete ctx; return LSA_E_HIP; }
  bool ok = true;
  ok &= hipStreamCreateWithFlags(&ctx->prefetch_stream, hipStreamNonBlocking) == hipSuccess;
  ok &= hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; i < 2; ++i) ok &= hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&ctx->ev_bbox, hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&ctx->ev_pred, hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&ctx->ev_stage, hipEventDisableTiming) == hipSuccess;
  ok &= hipMalloc((void**)&ctx->ring_start, (kMaxRings + 1) * sizeof(int)) == hipSuccess;
  ok &= hipMalloc((void**)&ctx->ring_len, kMaxRings * sizeof(int)) == hipSuccess;
  ok &= hipMalloc((void**)&ctx->extract_out, 16 * sizeof(int)) == hipSuccess;
  ok &= hipMalloc((void**)&ctx->extract_out_next, 16 * sizeof(int)) == hipSuccess;
  ok &= hipHostMalloc((void**)&ctx->host_next, 16 * sizeof(int), hipHostMallocDefault) == hipSuccess;
  ok &= hipEventCreateWithFlags(&ctx->ev_prefetch, hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&ctx->ev_spare, hipEventDisableTiming) == hipSuccess;
  for (int k = 0; k < 3; ++k) ok &= hipEventCreateWithFlags(&ctx->ev_map_ahead[k], hipEventDisableTiming) == hipSuccess;
  ok &= hipEventCreateWithFlags(&ctx->ev_kp_ready, hipEventDisableTiming) == hipSuccess;
  if (ok) { ctx->kp_count_dev = ctx->extract_out; ctx->ring_meta = ctx->extract_out + 4; }
  ok &= hipMalloc((void**)&ctx->ring_counts, kMaxRings * 3 * sizeof(int)) == hipSuccess;
  ok &= hipMalloc((void**)&ctx->partials, (size_t)kAccumBlocksMax * kAccumVals * sizeof(double)) == hipSuccess;
  ok &= hipMalloc((void**)&ctx->reduce_out, 64 * sizeof(double)) == hipSuccess;
  if (ok) ok &= hipMemset(ctx->reduce_out, 0, 64 * sizeof(double)) == hipSuccess;  // [32] holds the arrival ticket of k_accumulate
  ok &= hipMalloc((void**)&ctx->hist_dev, 3 * kHistRing * 16 * sizeof(int)) == hipSuccess;
  if (ok) ok &= hipMemset(ctx->hist_dev, 0, 3 * kHistRing * 16 * sizeof(int)) == hipSuccess;
  ok &= hipMalloc((void**)&ctx->range_bits, 48 * sizeof(unsigned long long)) == hipSuccess;
  ok &= hipHostMalloc((void**)&ctx->host_pinned, 512 * sizeof(double), hipHostMallocDefault) == hipSuccess;
  if (hipHostMalloc((void**)&ctx->mailbox, (size_t)kAccumBlocksMax * kMailboxStride * sizeof(unsigned long long), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess)
    std::memset(ctx->mailbox, 0, (size_t)kAccumBlocksMax * kMailboxStride * sizeof(unsigned long long));
  else
    ctx->mailbox = nullptr;  // optional: lsa_accumulate falls back to a copy + synchronise
  if (hipHostMalloc((void**)&ctx->lm_mailbox, (size_t)kLmMailRing * 2 * kLmOut * sizeof(unsigned long long), hipHostMallocCoherent | hipHostMallocMapped) == hipSuccess)
    std::memset(ctx->lm_mailbox, 0, (size_t)kLmMailRing * 2 * kLmOut * sizeof(unsigned long long));
  else
    ctx->lm_mailbox = nullptr;  // optional: lsa_solve_device then reports LSA_E_STATE and the host-driven loop is used
  // link blocks of ICP iterations enqueued ahead (lsa_icp_link): optional like the result mailbox
  if (ctx->lm_mailbox && (hipMalloc((void**)&ctx->link_dev, (size_t)kLinkRing * kLinkWords * sizeof(unsigned long long)) != hipSuccess ||
                          hipMemset(ctx->link_dev, 0, (size_t)kLinkRing * kLinkWords * sizeof(unsigned long long)) != hipSuccess))
    ctx->link_dev = nullptr;
  if (ctx->link_dev && (hipMalloc((void**)&ctx->motion_dev, 16 * sizeof(double)) != hipSuccess || hipMemset(ctx->motion_dev, 0, 16 * sizeof(double)) != hipSuccess))
    ctx->motion_dev = nullptr;  // optional: no links then (lsa_icp_link says so)
  ok &= hipMalloc((void**)&ctx->lm_xchg, (size_t)2 * kLmBlocksMax * kMailboxStride * sizeof(unsigned long long)) == hipSuccess;
  if (ok) ok &= hipMemset(ctx->lm_xchg, 0, (size_t)2 * kLmBlocksMax * kMailboxStride * sizeof(unsigned long long)) == hipSuccess;
  if (const char* e = std::getenv("LSA_ACCUM_BLOCKS")) ctx->accum_blocks = std::min(std::max(std::atoi(e), 1), kAccumBlocksMax);
  ctx->lm_cache_capacity = lm_cache_capacity();
  ctx->lm_cache_slots = ctx->lm_cache_capacity;
  if (const char* e = std::getenv("LSA_LM_CACHE")) ctx->lm_cache_slots = std::min(std::max(std::atoi(e), 0), ctx->lm_cache_slots);
  if (const char* e = std::getenv("LSA_LM_BLOCKS")) ctx->lm_blocks = std::min(std::max(std::atoi(e), 1), kLmBlocksMax);
  if (const char* e = std::getenv("LSA_LM_RECORDS")) ctx->lm_records = std::min(std::max(std::atoi(e), 256), 4096);
  if (const char* e = std::getenv("LSA_ROUTE_STATS")) ctx->route_stats = std::atoi(e) != 0;
  if (ctx->route_stats) ok &= hipMalloc(&ctx->trace_dev, ((size_t)8192 * 12 + 16) * sizeof(unsigned long long)) == hipSuccess && hipMemset(ctx->trace_dev, 0, ((size_t)8192 * 12 + 16) * sizeof(unsigned long long)) == hipSuccess;
  if (const char* e = std::getenv("LSA_FUSED_MATCH")) ctx->fused_match = std::atoi(e) != 0;
  if (const char* e = std::getenv("LSA_FUSED_MODEL")) ctx->fused_model = std::atoi(e) != 0;
  if (const char* e = std::getenv("LSA_MAILBOX_CHECK")) ctx->mailbox_check = std::atoi(e) != 0;
  ctx->created_knobs = {ctx->lm_blocks, ctx->lm_records, ctx->lm_cache_slots, ctx->accum_blocks, ctx->mailbox_check};
  if (!ok) { lsa_ctx_destroy(ctx); return LSA_E_HIP; }
  *out = ctx;
  return LSA_OK;
}

void lsa_ctx_destroy(lsa_ctx* ctx)
{
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (int i = 0; i < 2; ++i)
    if (ctx->side_stream[i]) (void)hipStreamSynchronize(ctx->side_stream[i]);
  if (ctx->prefetch_stream) (void)hipStreamSynchronize(ctx->prefetch_stream);
  if (ctx->uploader.joinable())
  {
    {
      std::lock_guard<std::mutex> l(ctx->up_mutex);
      ctx->up_quit = true;
    }
    ctx->up_cv.notify_all();
    ctx->up_help_cv.notify_all();
    ctx->up_help_done.notify_all();
    ctx->uploader.join();
    for (auto& h : ctx->up_helpers) h.join();
    ctx->up_helpers.clear();
  }
  (void)lsa_collect_garbage(ctx);
  if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
  for (auto& in : ctx->inbox)
  {
    if (in.dev) (void)hipFree(in.dev);
    if (in.pinned) (void)hipHostFree(in.pinned);
    if (in.ev) (void)hipEventDestroy(in.ev);
  }
  profile_collect(ctx);
  for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
  auto fr = [](void* p) { if (p) (void)hipFree(p); };
  fr(ctx->frame_own); fr(ctx->xyzi); fr(ctx->orig); fr(ctx->ring_of); fr(ctx->block_hist);
  fr(ctx->ring_start); fr(ctx->ring_len); fr(ctx->extract_out); fr(ctx->extract_out_next);
  for (int k = 0; k < 3; ++k) fr(ctx->kp_next[k]);
  if (ctx->host_next) (void)hipHostFree(ctx->host_next);
  if (ctx->ev_prefetch) (void)hipEventDestroy(ctx->ev_prefetch);
  if (ctx->ev_spare) (void)hipEventDestroy(ctx->ev_spare);
  for (int k = 0; k < 3; ++k)
    if (ctx->ev_map_ahead[k]) (void)hipEventDestroy(ctx->ev_map_ahead[k]);
  if (ctx->ev_kp_ready) (void)hipEventDestroy(ctx->ev_kp_ready);
  if (ctx->ev_dense) (void)hipEventDestroy(ctx->ev_dense);
  if (ctx->prefetch_stream) (void)hipStreamDestroy(ctx->prefetch_stream);
  for (int i = 0; i < 4; ++i) fr(ctx->score[i]);
  fr(ctx->valid); fr(ctx->label); fr(ctx->ring_counts);
  for (int s = 0; s < 3; ++s) for (int k = 0; k < 3; ++k) fr(ctx->kp[s][k]);
  for (int k = 0; k < 12; ++k)
  {
    Target& t = ctx->target[k];
    fr(t.pts); fr(t.xyzl); fr(t.desc); fr(t.bbox_bits);
    for (int l = 0; l < kGridLevels; ++l) { fr(t.lv[l].sorted); fr(t.lv[l].cell_of); fr(t.lv[l].cell_start); fr(t.lv[l].cell_fill); fr(t.lv[l].block_sums); }
  }
  for (int k = 0; k < 3; ++k)
  {
    fr(ctx->match[k].rec); fr(ctx->match[k].status); fr(ctx->match[k].knn_idx); fr(ctx->match[k].knn_d2); fr(ctx->match[k].knn_cnt); fr(ctx->match[k].slow_list); fr(ctx->match[k].slow_pts);
  }
  kplog_destroy(ctx);
  pgo_destroy(ctx);
  map_place_destroy(ctx);
  fr(ctx->place_results.dev);
  if (ctx->place_results.pinned) (void)hipHostFree(ctx->place_results.pinned);
  fr(ctx->partials); fr(ctx->reduce_out); fr(ctx->hist_dev); fr(ctx->scratch_out); fr(ctx->range_bits);
  for (auto& s : ctx->store) fr(s.first);
  if (ctx->host_pinned) (void)hipHostFree(ctx->host_pinned);
  if (ctx->mailbox) (void)hipHostFree(ctx->mailbox);
  if (ctx->lm_mailbox) (void)hipHostFree(ctx->lm_mailbox);
  fr(ctx->link_dev);
  fr(ctx->motion_dev);
  fr(ctx->lm_xchg);
  fr(ctx->trace_dev);
  for (int i = 0; i < 2; ++i)
  {
    if (ctx->ev_join[i]) (void)hipEventDestroy(ctx->ev_join[i]);
    if (ctx->side_stream[i]) (void)hipStreamDestroy(ctx->side_stream[i]);
  }
  if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
  if (ctx->ev_bbox) (void)hipEventDestroy(ctx->ev_bbox);
  if (ctx->ev_pred) (void)hipEventDestroy(ctx->ev_pred);
  if (ctx->ev_stage) (void)hipEventDestroy(ctx->ev_stage);
  for (int k = 0; k < 3; ++k)
    if (ctx->stage[k]) (void)hipHostFree(ctx->stage[k]);
  for (int b = 0; b < 2; ++b)
  {
    if (ctx->pcd_pinned[b]) (void)hipHostFree(ctx->pcd_pinned[b]);
    if (ctx->pcd_dev[b]) (void)hipFree(ctx->pcd_dev[b]);
    if (ctx->pcd_ev_copy[b]) (void)hipEventDestroy(ctx->pcd_ev_copy[b]);
    if (ctx->pcd_ev_kernel[b]) (void)hipEventDestroy(ctx->pcd_ev_kernel[b]);
  }
  for (int k = 0; k < 6; ++k)
    if (ctx->tstage[k]) (void)hipHostFree(ctx->tstage[k]);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  g_live_contexts.fetch_sub(1, std::memory_order_relaxed);
  delete ctx;
}

const char* lsa_last_error(const lsa_ctx* ctx)
{
  if (!ctx) return "null context";
  // a copy of the calling thread's own: another thread of the pipeline may report an error meanwhile
  thread_local std::string copy;
  {
    std::lock_guard<std::mutex> l(ctx->error_mutex);
    copy = ctx->error;
  }
  return copy.c_str();
}

int lsa_sync(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

// The host threads of a context talk to the device in tens of short round trips per frame (mailbox polls, pinned
// staging buffers): on a two-socket host they belong on the socket the GPU hangs off.
int lsa_bind_host_to_device(int device_id)
{
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), device_id) != hipSuccess) return LSA_E_NO_DEVICE;
  for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
  int node = -1;
  {
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
    if (FILE* f = std::fopen(path.c_str(), "r")) { if (std::fscanf(f, "%d", &node) != 1) node = -1; std::fclose(f); }
  }
  if (node < 0) return LSA_E_STATE;  // single-socket host, or the kernel does not say
  cpu_set_t want;
  CPU_ZERO(&want);
  {
    const std::string path = "/sys/devices/system/node/node" + std::to_string(node) + "/cpulist";
    FILE* f = std::fopen(path.c_str(), "r");
    if (!f) return LSA_E_STATE;
    int a = 0, b = 0;
    // "0-63,128-191"
    while (std::fscanf(f, "%d", &a) == 1)
    {
      b = a;
      int ch = std::fgetc(f);
      if (ch == '-') { if (std::fscanf(f, "%d", &b) != 1) b = a; ch = std::fgetc(f); }
      for (int c = a; c <= b && c < CPU_SETSIZE; ++c) CPU_SET(c, &want);
      if (ch != ',') break;
    }
    std::fclose(f);
  }
  cpu_set_t have;
  CPU_ZERO(&have);
  if (sched_getaffinity(0, sizeof(have), &have) != 0) return LSA_E_STATE;
  cpu_set_t both;
  CPU_AND(&both, &want, &have);
  if (CPU_COUNT(&both) == 0) return LSA_E_STATE;  // the node's CPUs are not ours to use
  if (sched_setaffinity(0, sizeof(both), &both) != 0) return LSA_E_STATE;
  return node;
}

int lsa_frame_size(const lsa_ctx* ctx) { return ctx ? ctx->frame_n : 0; }
int lsa_download_frame(lsa_ctx* ctx, lsa_point_t* out, int capacity)
{
  if (!ctx || !out) return ctx ? ctx->fail(LSA_E_ARG, "lsa_download_frame: null argument") : LSA_E_ARG;
  if (!ctx->frame || ctx->frame_n <= 0) return ctx->fail(LSA_E_STATE, "lsa_download_frame: no frame");
  if (capacity < ctx->frame_n) return ctx->fail(LSA_E_CAPACITY, "lsa_download_frame: capacity < frame size");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, hipMemcpyAsync(out, ctx->frame, (size_t)ctx->frame_n * sizeof(lsa_point_t), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ctx->frame_n;
}
float lsa_get_azimuthal_resolution(const lsa_ctx* ctx) { return ctx ? ctx->az_res : 0.f; }
void lsa_set_azimuthal_resolution(lsa_ctx* ctx, float rad) { if (ctx) ctx->az_res = rad; }
int lsa_nb_laser_rings(const lsa_ctx* ctx) { return ctx ? ctx->nb_rings_seen : 0; }

}  // extern "C"
