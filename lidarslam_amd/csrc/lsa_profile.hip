// lsa_profile.hip -- per-kernel HIP-event profiling: the scopes around the launches and the C ABI that reads them.
#include <algorithm>
#include "lsa_ctx.h"

using namespace lsa;

namespace lsa
{

ProfScope::ProfScope(lsa_ctx* c, const char* name, double bytes, hipStream_t stream) : ctx(c), st(stream ? stream : c->stream)
{
  if (!ctx->profiling) return;
  // a selection names a scope or a family of scopes by their common prefix ("match_": match_search and match_model); the
  // sixty other scopes of a frame leave at once (prof_only is set while nothing is being enqueued: lsa_profile_select)
  if (!ctx->prof_only.empty() && std::strncmp(name, ctx->prof_only.c_str(), ctx->prof_only.size()) != 0) return;
  std::lock_guard<std::mutex> lock(ctx->prof_mutex);  // the device maps' insertions are enqueued (and timed) by other host threads
  for (size_t i = 0; i < ctx->stats.size(); ++i)
    if (ctx->stats[i].name == name) { stat = (int)i; break; }
  if (stat < 0)
  {
    KernelStat ks;
    ks.name = name;
    ctx->stats.push_back(ks);
    stat = (int)ctx->stats.size() - 1;
  }
  ctx->stats[stat].launches++;
  ctx->stats[stat].bytes += bytes;
  if (ctx->prof_every > 1 && (ctx->stats[stat].launches % ctx->prof_every) != 1) { stat = -1; return; }
  ctx->stats[stat].timed++;
  auto get = [&]() {
    hipEvent_t e;
    if (!ctx->event_pool.empty()) { e = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
  };
  a = get();
  b = get();
  (void)hipEventRecord(a, st);
}
ProfScope::~ProfScope()
{
  if (stat < 0) return;
  (void)hipEventRecord(b, st);
  std::lock_guard<std::mutex> lock(ctx->prof_mutex);
  ctx->pending.push_back({stat, a, b});
}
void profile_add_bytes(lsa_ctx* ctx, const char* name, double bytes)
{
  if (!ctx->profiling) return;
  std::lock_guard<std::mutex> lock(ctx->prof_mutex);
  for (auto& st : ctx->stats)
    if (st.name == name) { st.bytes += bytes; return; }
}

void profile_collect(lsa_ctx* ctx)
{
  std::lock_guard<std::mutex> lock(ctx->prof_mutex);
  for (auto& p : ctx->pending)
  {
    (void)hipEventSynchronize(p.b);
    float ms = 0;
    if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) ctx->stats[p.stat].total_ms += std::max(0.0, (double)ms - ctx->prof_overhead_ms);
    ctx->event_pool.push_back(p.a);
    ctx->event_pool.push_back(p.b);
  }
  ctx->pending.clear();
}

}  // namespace lsa

extern "C" {

// what two events measure with nothing between them (the markers' own way through the queue): the median of 15 pairs on the
// idle stream.  A scope's time is what its events measure minus this, so that it can be held against a profiler's figure
// for the kernel alone.
static void calibrate_event_overhead(lsa_ctx* ctx)
{
  if (ctx->prof_overhead_ms > 0.) return;
  hipEvent_t a = nullptr, b = nullptr;
  if (hipSetDevice(ctx->device) != hipSuccess || hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
  (void)hipStreamSynchronize(ctx->stream);
  std::vector<float> ms;
  for (int i = 0; i < 15; ++i)
  {
    (void)hipEventRecord(a, ctx->stream);
    (void)hipEventRecord(b, ctx->stream);
    (void)hipEventSynchronize(b);
    float t = 0;
    if (hipEventElapsedTime(&t, a, b) == hipSuccess) ms.push_back(t);
  }
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  if (ms.empty()) return;
  std::sort(ms.begin(), ms.end());
  ctx->prof_overhead_ms = ms[ms.size() / 2];
}

double lsa_profile_event_overhead_us(const lsa_ctx* ctx) { return ctx ? 1e3 * ctx->prof_overhead_ms : 0.; }

int lsa_profile_enable(lsa_ctx* ctx, int on)
{
  if (!ctx) return LSA_E_ARG;
  if (on) calibrate_event_overhead(ctx);
  ctx->profiling = on != 0;
  ctx->prof_only.clear();
  ctx->prof_every = 1;
  return LSA_OK;
}
int lsa_profile_select(lsa_ctx* ctx, const char* scope, int every)
{
  if (!ctx || !scope || every < 1) return LSA_E_ARG;
  calibrate_event_overhead(ctx);
  ctx->profiling = true;
  ctx->prof_only = scope;
  ctx->prof_every = every;
  return LSA_OK;
}
int lsa_profile_reset(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  profile_collect(ctx);
  ctx->stats.clear();
  return LSA_OK;
}
int lsa_profile_get(lsa_ctx* ctx, lsa_kernel_stat_t* out, int capacity)
{
  if (!ctx) return LSA_E_ARG;
  (void)hipStreamSynchronize(ctx->stream);
  profile_collect(ctx);
  int n = std::min<int>(capacity, ctx->stats.size());
  for (int i = 0; i < n; ++i)
  {
    std::memset(&out[i], 0, sizeof(out[i]));
    std::strncpy(out[i].name, ctx->stats[i].name.c_str(), sizeof(out[i].name) - 1);
    out[i].launches = ctx->stats[i].launches;
    // sampled scopes: the timed launches' mean stands for all launches
    out[i].total_ms = ctx->stats[i].timed > 0 ? ctx->stats[i].total_ms * ((double)ctx->stats[i].launches / ctx->stats[i].timed) : 0.;
    out[i].bytes = ctx->stats[i].bytes;
  }
  return n;
}

}  // extern "C"
