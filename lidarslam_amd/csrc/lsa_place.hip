// lsa_place.hip -- place recognition on the keypoint log: a descriptor per logged frame, kept in a store that follows the log
// (DESIGN.md 3.8).  The definition is lsa_scan_descriptor.h, the text the host statement (host/lsa_place.cpp) compiles too;
// the kernel below decides only who computes what.  The comparison of one frame's descriptor with a range of others is
// lsa_place_search.hip's k_place_search.
//   k_log_describe   a workgroup per frame: its keypoints binned into an LDS image of the cells by atomic max on ordered
//                    words, then a lane per sector for the column norms (lsa_place_image.h)
// The descriptor store belongs to the log: a ring of slots, frame i in slot (head + i) % capacity, so that dropping the
// oldest frame moves nothing.  Filled lazily; follows lsa_kplog_append / _pop_front / _clear (lsa_kplog.hip tells it); a
// change of any parameter invalidates it; nothing is freed while work may be in flight (the context's graveyard).
#include <algorithm>
#include <deque>
#include <vector>
#include "lsa_ctx.h"
#include "lsa_kplog_io.h"
#include "lsa_place_image.h"
#include "lsa_place_io.h"

using namespace lsa;

namespace lsa
{
void place_pop_front(lsa_ctx* ctx)
{
  PlaceStore* st = ctx->place;
  if (!st) return;
  if (st->valid.empty()) { st->head = 0; return; }
  st->valid.pop_front();
  st->head = st->cap > 0 ? (st->head + 1) % st->cap : 0;
}
void place_clear(lsa_ctx* ctx)
{
  PlaceStore* st = ctx->place;
  if (!st) return;
  st->valid.clear();
  st->head = 0;
}
void place_destroy(lsa_ctx* ctx)
{
  PlaceStore* st = ctx->place;
  if (!st) return;
  if (st->slots) (void)hipFree(st->slots);
  if (st->table) (void)hipFree(st->table);
  if (st->rows_table) (void)hipFree(st->rows_table);
  if (st->detect_up_dev) (void)hipFree(st->detect_up_dev);
  if (st->detect_up_host) (void)hipHostFree(st->detect_up_host);
  if (st->detect_res_dev) (void)hipFree(st->detect_res_dev);
  if (st->detect_res_host) (void)hipHostFree(st->detect_res_host);
  delete st;
  ctx->place = nullptr;
}
}  // namespace lsa

namespace
{
constexpr int kDescribeThreads = 256;

// A workgroup per frame: the image of the cells in LDS, finished in place.
__global__ __launch_bounds__(kDescribeThreads) void k_log_describe(const DescribeFrame* __restrict__ frames, float* __restrict__ slots, int stride, lsa_place_params_t p)
{
  __shared__ unsigned s_img[kImageCells];
  const DescribeFrame f = frames[blockIdx.x];
  const int cells = p.rings * p.sectors;  // <= kImageCells: the parameters were checked
  for (int c = threadIdx.x; c < cells; c += kDescribeThreads) s_img[c] = 0u;
  __syncthreads();
  for (int t = 0; t < 3; ++t)
    for (int i = threadIdx.x; i < f.n[t]; i += kDescribeThreads)
    {
      const float4 a = f.pts[t][2 * (size_t)i];
      image_offer(s_img, p, a.x, a.y, a.z);
    }
  __syncthreads();
  image_finish<kDescribeThreads>(s_img, reinterpret_cast<float*>(s_img), slots + (size_t)f.slot * (size_t)stride, p);
}
}  // namespace

namespace lsa
{
void place_describe_launch(const DescribeFrame* frames_dev, int count, float* slots, int stride, const lsa_place_params_t& p, hipStream_t stream)
{
  hipLaunchKernelGGL(k_log_describe, dim3((unsigned)count), dim3(kDescribeThreads), 0, stream, frames_dev, slots, stride, p);
}
}  // namespace lsa

namespace
{
int check(lsa_ctx* ctx, const char* who, const lsa_place_params_t* params, int first, int last)
{
  if (!ctx) return LSA_E_ARG;
  if (int rc = check_params(ctx, who, params)) return rc;
  if (lsa_kplog_stopped(ctx)) return ctx->fail(LSA_E_STATE, std::string(who) + ": keypoint logging stopped when a chunk could not be allocated");
  const int n = lsa_kplog_size(ctx);
  if (first < 0 || last < first || last >= n)
    return ctx->fail(LSA_E_ARG, std::string(who) + ": frames " + std::to_string(first) + ".." + std::to_string(last) + " of " + std::to_string(n) + " logged ones");
  return LSA_OK;
}

// the store for these parameters with a slot for every logged frame; what it held under other parameters is forgotten
int ensure_store(lsa_ctx* ctx, const lsa_place_params_t& p)
{
  if (!ctx->place) ctx->place = new PlaceStore;
  PlaceStore* st = ctx->place;
  const long long n = lsa_kplog_size(ctx);
  if (!st->have_params || !same_params(st->params, p))
  {
    st->params = p;
    st->have_params = true;
    st->valid.clear();
    st->head = 0;
    if (st->stride != place::length(p))
    {
      retire_dev(ctx, st->slots);
      st->slots = nullptr;
      st->cap = 0;
      st->stride = place::length(p);
    }
  }
  if (n > st->cap)
  {
    const long long cap = std::max<long long>(n + n / 2, 64);
    float* slots = nullptr;
    LSA_HIP(ctx, hipMalloc((void**)&slots, (size_t)cap * (size_t)st->stride * sizeof(float)));
    // what is held moves to the front of the new ring, behind whatever still writes it on the context's stream
    const long long m = (long long)st->valid.size();
    if (st->slots && m > 0)
    {
      const size_t slot_bytes = (size_t)st->stride * sizeof(float);
      const long long run = std::min(m, st->cap - st->head);
      hipError_t e = hipMemcpyAsync(slots, st->slots + (size_t)st->head * st->stride, (size_t)run * slot_bytes, hipMemcpyDeviceToDevice, ctx->stream);
      if (e == hipSuccess && m > run) e = hipMemcpyAsync(slots + (size_t)run * st->stride, st->slots, (size_t)(m - run) * slot_bytes, hipMemcpyDeviceToDevice, ctx->stream);
      if (e != hipSuccess)
      {
        (void)hipFree(slots);
        return ctx->fail(LSA_E_HIP, std::string("lsa_place: moving the descriptor store: ") + hipGetErrorString(e));
      }
    }
    retire_dev(ctx, st->slots);
    st->slots = slots;
    st->cap = cap;
    st->head = 0;
  }
  return LSA_OK;
}

// describes those of the frames first..last, and of `also` (< 0: none), that have no valid descriptor: one launch
int describe_missing(lsa_ctx* ctx, PlaceStore* st, int first, int last, int also)
{
  const lsa_place_params_t& p = st->params;
  const int n = lsa_kplog_size(ctx);
  if ((int)st->valid.size() < n) st->valid.resize((size_t)n, 0);
  std::vector<DescribeFrame> frames;
  std::vector<int> which;
  long long points = 0;
  auto take = [&](int i) {
    if (st->valid[(size_t)i]) return;
    const lsa_point_t* pts[3];
    int cnt[3];
    if (!kplog_frame(ctx, i, pts, cnt)) return;
    DescribeFrame f;
    for (int k = 0; k < 3; ++k)
    {
      const bool used = (p.type_mask >> k) & 1u;
      f.pts[k] = reinterpret_cast<const float4*>(pts[k]);
      f.n[k] = used ? cnt[k] : 0;
      points += f.n[k];
    }
    f.slot = (int)((st->head + i) % st->cap);
    frames.push_back(f);
    which.push_back(i);
  };
  for (int i = first; i <= last; ++i) take(i);
  if (also >= 0 && (also < first || also > last)) take(also);
  st->described = 0;
  if (frames.empty()) return LSA_OK;
  const size_t bytes = frames.size() * sizeof(DescribeFrame);
  if (int rc = scratch_room<char>(ctx, &st->table, nullptr, &st->table_cap, bytes)) return rc;
  LSA_HIP(ctx, hipMemcpyAsync(st->table, frames.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
  {
    ProfScope ps(ctx, "log_describe", (double)points * 32 + (double)frames.size() * ((double)st->stride * 4 + sizeof(DescribeFrame)));
    place_describe_launch(reinterpret_cast<const DescribeFrame*>(st->table), (int)frames.size(), st->slots, st->stride, p, ctx->stream);
  }
  LSA_HIP(ctx, hipGetLastError());
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `frames` goes away
  for (int i : which) st->valid[(size_t)i] = 1;
  st->described = (int)which.size();
  return LSA_OK;
}
}  // namespace

namespace lsa
{
int place_prepare(lsa_ctx* ctx, const char* who, const lsa_place_params_t* params, int first, int last)
{
  int rc = check(ctx, who, params, first, last);
  if (rc) return rc;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  rc = ensure_store(ctx, *params);
  if (rc) return rc;
  return describe_missing(ctx, ctx->place, first, last, -1);
}
}  // namespace lsa

extern "C" {

int lsa_kplog_describe(lsa_ctx* ctx, const lsa_place_params_t* params, int first, int last)
{
  const int rc = place_prepare(ctx, "lsa_kplog_describe", params, first, last);
  return rc ? rc : ctx->place->described;
}

int lsa_kplog_described(const lsa_ctx* ctx) { return ctx && ctx->place ? ctx->place->described : 0; }

int lsa_kplog_descriptor_length(const lsa_ctx* ctx) { return ctx && ctx->place && ctx->place->have_params ? ctx->place->stride : 0; }

int lsa_kplog_descriptors(lsa_ctx* ctx, int first, int last, float* out)
{
  if (!ctx) return LSA_E_ARG;
  const int n = lsa_kplog_size(ctx);
  if (!out || first < 0 || last < first || last >= n) return ctx->fail(LSA_E_ARG, "lsa_kplog_descriptors: bad argument");
  PlaceStore* st = ctx->place;
  bool all = st && (int)st->valid.size() > last;
  for (int i = first; all && i <= last; ++i) all = st->valid[(size_t)i] != 0;
  if (!all) return ctx->fail(LSA_E_STATE, "lsa_kplog_descriptors: a frame of the range has not been described (lsa_kplog_describe)");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const size_t slot_bytes = (size_t)st->stride * sizeof(float);
  const long long m = (long long)last - first + 1, at = (st->head + first) % st->cap;
  const long long run = std::min(m, st->cap - at);
  LSA_HIP(ctx, hipMemcpyAsync(out, st->slots + (size_t)at * st->stride, (size_t)run * slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (m > run) LSA_HIP(ctx, hipMemcpyAsync(out + (size_t)run * st->stride, st->slots, (size_t)(m - run) * slot_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

int lsa_kplog_place_search(lsa_ctx* ctx, const lsa_place_params_t* params, int query, int first, int last, float* distance_out, int32_t* shift_out)
{
  const char* who = "lsa_kplog_place_search";
  int rc = check(ctx, who, params, first, last);
  if (rc) return rc;
  if (!distance_out || !shift_out) return ctx->fail(LSA_E_ARG, std::string(who) + ": bad argument");
  if (query < 0 || query >= lsa_kplog_size(ctx)) return ctx->fail(LSA_E_ARG, std::string(who) + ": query frame " + std::to_string(query) + " is not a logged one");
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  rc = ensure_store(ctx, *params);
  if (rc) return rc;
  PlaceStore* st = ctx->place;
  rc = describe_missing(ctx, st, first, last, query);
  if (rc) return rc;
  return place_search_one(ctx, st->slots, st->cap, st->head, st->stride, st->params, query, first, last - first + 1, distance_out, shift_out);
}

}  // extern "C"
