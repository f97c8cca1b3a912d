// lsa_place.hip -- place recognition on the keypoint log: a descriptor per logged frame, and the exhaustive comparison of one
// frame's descriptor with a range of others.  The definition of both is lsa_scan_descriptor.h, the text the
// host statement (host/lsa_place.cpp) compiles too; the kernels below decide only who computes what.
//   k_log_describe   a workgroup per frame: its keypoints binned into an LDS image of the cells by atomic max on ordered
//                    words, then a lane per sector for the column norms
//   k_place_search   a workgroup per candidate: both descriptors in LDS, the cosines of a tile of shifts across the lanes,
//                    a lane per shift for the sums in the fixed column order, one (distance, shift) per candidate
// The descriptor store belongs to the log: a ring of slots, frame i in slot (head + i) % capacity, so that dropping the
// oldest frame moves nothing.  Filled lazily; follows lsa_kplog_append / _pop_front / _clear (lsa_kplog.hip tells it); a
// change of any parameter invalidates it; nothing is freed while work may be in flight (the context's graveyard).
#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>
#include "lsa_ctx.h"
#include "lsa_kplog_io.h"
#include "lsa_place_io.h"
#include "lsa_scan_descriptor.h"
#include "lsa_wave.h"

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
  if (st->result_dev) (void)hipFree(st->result_dev);
  if (st->result_host) (void)hipHostFree(st->result_host);
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
constexpr int kSearchThreads = 256;
constexpr int kShiftTile = 64;          // shifts whose cosines are in LDS at a time: one wavefront sums them
constexpr int kSearchBlocks = 2048;     // of a launch, unless lsa_debug_set "place_max_blocks" says otherwise
constexpr int kMaxCells = place::kMaxRings * place::kMaxSectors;
constexpr int kMaxLength = kMaxCells + place::kMaxSectors;
// k_place_search's LDS at the largest shape: two descriptors and a tile of cosines with rows of an odd length
static_assert((2 * kMaxLength + kShiftTile * (place::kMaxSectors | 1)) * sizeof(float) <= 64 * 1024, "k_place_search keeps to 64 KB of LDS");

// A workgroup per frame.  The image of the cells is LDS words in the order-preserving coding of floats (f2ou), 0 = no
// point yet (no float codes to 0 but a NaN, and a NaN takes no part), so the largest offer of a cell is one LDS atomic max
// per point whatever the order.  Then a thread per cell turns the word into the cell's value, writes it and leaves it in
// LDS as a float for the norms: a lane per sector, rings ascending.
__global__ __launch_bounds__(kDescribeThreads) void k_log_describe(const DescribeFrame* __restrict__ frames, float* __restrict__ slots, int stride, lsa_place_params_t p)
{
  __shared__ unsigned s_img[kMaxCells];
  const DescribeFrame f = frames[blockIdx.x];
  const int cells = p.rings * p.sectors;  // <= kMaxCells: the parameters were checked
  for (int c = threadIdx.x; c < cells; c += kDescribeThreads) s_img[c] = 0u;
  __syncthreads();
  for (int t = 0; t < 3; ++t)
    for (int i = threadIdx.x; i < f.n[t]; i += kDescribeThreads)
    {
      const float4 a = f.pts[t][2 * (size_t)i];
      int cell;
      if (place::cell_of(p, a.x, a.y, a.z, &cell)) atomicMax(&s_img[cell], f2ou(place::offer(p, a.z)));
    }
  __syncthreads();
  float* __restrict__ out = slots + (size_t)f.slot * (size_t)stride;
  for (int c = threadIdx.x; c < cells; c += kDescribeThreads)
  {
    const unsigned u = s_img[c];
    const float v = u ? place::cell_value(ou2f(u)) : 0.f;
    out[c] = v;
    s_img[c] = __float_as_uint(v);
  }
  __syncthreads();
  const float* img = reinterpret_cast<const float*>(s_img);
  for (int j = threadIdx.x; j < p.sectors; j += kDescribeThreads) out[cells + j] = place::column_norm(img, p.rings, p.sectors, j);
}

struct SearchArgs
{
  const float* slots;
  PlaceResult* out;     // [count]
  long long cap, head;  // the store's ring
  int stride;
  int query, first, count;  // frames: the candidates are first .. first + count - 1
};

// A workgroup per candidate, striding over the range.  LDS: q and c whole (cells and norms), and the cosines of kShiftTile
// shifts, row = shift, rows of an odd length: the lanes that sum -- one per shift, each walking its row in column order, all
// at the same column -- then sit on distinct banks.  The cosines of a tile are spread over all lanes, column fastest, so
// q's reads are consecutive and c's consecutive up to the wrap.  A column that is empty in q or in c has no cosine; the
// summing lane tests the norms again rather than a marker in the table.  Lane s keeps the best of its shifts s, s + 64 (tiles
// ascending, so an equal distance never displaces the lower shift); the first wavefront reduces by shuffles with the same
// rule, which is a total order: any tree gives the sequential loop's answer.
__global__ __launch_bounds__(kSearchThreads) void k_place_search(SearchArgs a, lsa_place_params_t p)
{
  extern __shared__ float s_lds[];
  const int rings = p.rings, sectors = p.sectors, cells = rings * sectors, length = cells + sectors;
  const int row = sectors | 1;
  const int minCommon = place::min_common(p);
  float* q = s_lds;
  float* c = q + length;
  float* tab = c + length;
  const float* nq = q + cells;
  const float* nc = c + cells;
  {
    const float* __restrict__ src = a.slots + (size_t)((a.head + a.query) % a.cap) * (size_t)a.stride;
    for (int i = threadIdx.x; i < length; i += kSearchThreads) q[i] = src[i];
  }
  for (int b = blockIdx.x; b < a.count; b += gridDim.x)
  {
    __syncthreads();  // the last candidate's readers of c are done (and q is there)
    const float* __restrict__ src = a.slots + (size_t)((a.head + a.first + b) % a.cap) * (size_t)a.stride;
    for (int i = threadIdx.x; i < length; i += kSearchThreads) c[i] = src[i];
    __syncthreads();
    float best = 0.f;
    int bestShift = -1;
    for (int s0 = 0; s0 < sectors; s0 += kShiftTile)
    {
      const int ts = min(kShiftTile, sectors - s0);
      for (int e = threadIdx.x; e < ts * sectors; e += kSearchThreads)
      {
        const int sl = e / sectors, j = e - sl * sectors;
        int k = j + s0 + sl;
        if (k >= sectors) k -= sectors;
        const float nqj = nq[j], nck = nc[k];
        tab[sl * row + j] = (nqj > 0.f && nck > 0.f) ? place::cosine(q, c, rings, sectors, j, k, nqj, nck) : 0.f;
      }
      __syncthreads();
      if ((int)threadIdx.x < ts)
      {
        const int s = s0 + threadIdx.x;
        const float* mine = tab + threadIdx.x * row;
        float sum = 0.f;
        int cnt = 0;
        for (int j = 0; j < sectors; ++j)
        {
          int k = j + s;
          if (k >= sectors) k -= sectors;
          if (nq[j] > 0.f && nc[k] > 0.f)
          {
            sum += mine[j];
            ++cnt;
          }
        }
        const float d = place::shift_distance(sum, cnt, minCommon);
        if (bestShift < 0 || place::beats(d, s, best, bestShift)) { best = d; bestShift = s; }
      }
      __syncthreads();  // before the next tile overwrites the table
    }
    if (threadIdx.x < 64)
    {
      for (int off = 32; off > 0; off >>= 1)
      {
        const float d2 = __shfl_down(best, off);
        const int s2 = __shfl_down(bestShift, off);
        if (s2 >= 0 && (bestShift < 0 || place::beats(d2, s2, best, bestShift))) { best = d2; bestShift = s2; }
      }
      if (threadIdx.x == 0) a.out[b] = PlaceResult{best, bestShift};
    }
  }
}

}  // namespace

namespace lsa
{
void place_describe_launch(const DescribeFrame* frames_dev, int count, float* slots, int stride, const lsa_place_params_t& p, hipStream_t stream)
{
  hipLaunchKernelGGL(k_log_describe, dim3((unsigned)count), dim3(kDescribeThreads), 0, stream, frames_dev, slots, stride, p);
}
void place_search_launch(lsa_ctx* ctx, const float* slots, long long cap, long long head, int stride, int query, int first, int count, PlaceResult* out_dev,
                         const lsa_place_params_t& p, hipStream_t stream)
{
  const size_t lds = (size_t)(2 * place::length(p) + kShiftTile * (p.sectors | 1)) * sizeof(float);  // <= 64 KB (the static_assert above)
  const int blocks = std::min(count, ctx->place_max_blocks > 0 ? ctx->place_max_blocks : kSearchBlocks);
  SearchArgs a;
  a.slots = slots;
  a.out = out_dev;
  a.cap = cap;
  a.head = head;
  a.stride = stride;
  a.query = query;
  a.first = first;
  a.count = count;
  hipLaunchKernelGGL(k_place_search, dim3((unsigned)blocks), dim3(kSearchThreads), lds, stream, a, p);
}
}  // namespace lsa

namespace
{
int check(lsa_ctx* ctx, const char* who, const lsa_place_params_t* params, int first, int last)
{
  if (!ctx) return LSA_E_ARG;
  if (!params || !place::params_ok(*params)) return ctx->fail(LSA_E_ARG, std::string(who) + ": descriptor parameters out of limits");
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
  static_assert(sizeof(lsa_place_params_t) == 4 * sizeof(int32_t) + 3 * sizeof(double), "no padding: compared by bytes");
  if (!st->have_params || std::memcmp(&st->params, &p, sizeof(p)) != 0)
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
  if (bytes > st->table_cap)
  {
    retire_dev(ctx, st->table);
    st->table = nullptr;
    st->table_cap = 0;
    LSA_HIP(ctx, hipMalloc(&st->table, bytes + bytes / 2));
    st->table_cap = bytes + bytes / 2;
  }
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
  int rc = check(ctx, "lsa_kplog_describe", params, first, last);
  if (rc) return rc;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  rc = ensure_store(ctx, *params);
  if (rc) return rc;
  rc = describe_missing(ctx, ctx->place, first, last, -1);
  if (rc) return rc;
  return ctx->place->described;
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
  const long long count = (long long)last - first + 1;
  if (count > st->result_cap)
  {
    retire_dev(ctx, st->result_dev);
    retire_host(ctx, st->result_host);
    st->result_dev = nullptr;
    st->result_host = nullptr;
    st->result_cap = 0;
    const long long cap = count + count / 2;
    LSA_HIP(ctx, hipMalloc((void**)&st->result_dev, (size_t)cap * sizeof(PlaceResult)));
    LSA_HIP(ctx, hipHostMalloc((void**)&st->result_host, (size_t)cap * sizeof(PlaceResult), hipHostMallocDefault));
    st->result_cap = cap;
  }
  const lsa_place_params_t& p = st->params;
  const int length = place::length(p);
  {
    ProfScope ps(ctx, "place_search", (double)(count + 1) * length * 4 + (double)count * sizeof(PlaceResult));
    place_search_launch(ctx, st->slots, st->cap, st->head, st->stride, query, first, (int)count, st->result_dev, p, ctx->stream);
  }
  LSA_HIP(ctx, hipGetLastError());
  LSA_HIP(ctx, hipMemcpyAsync(st->result_host, st->result_dev, (size_t)count * sizeof(PlaceResult), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (long long i = 0; i < count; ++i)
  {
    distance_out[i] = st->result_host[i].distance;
    shift_out[i] = st->result_host[i].shift;
  }
  return LSA_OK;
}

}  // extern "C"
