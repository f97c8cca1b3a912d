// lsa_place_search.hip -- the distance of two descriptors on the device, for every place call.  The
// distance is lsa_scan_descriptor.h's, the text the host statement (host/lsa_place.cpp) compiles too; the kernels below decide
// only who computes what, and both are held to it byte for byte.  Two launch shapes, because each loses to the other on the
// other's ground (DESIGN.md 3.8 has the figures):
//   k_place_search        one query against a range -- a frame of the log (lsa_place.hip), the viewpoints of the maps
//                         (lsa_map_place.hip).  A workgroup per candidate: both descriptors in LDS, the cosines of a tile of
//                         shifts across all lanes, a lane per shift for the sums in the fixed column order.  The shortest way
//                         to ONE pair's distance: what a call with a few or a few hundred candidates waits for
//   k_place_search_rows   loop detection (lsa_place_detect.hip): the ragged table of a run of queries, row k = (distance, shift)
//                         of query q_k against the frames 0 .. len_k - 1.  A workgroup walks a contiguous piece of the run's
//                         tiles (a tile: the pairs in flight, consecutive candidates of one query), so the query's descriptor
//                         stays in LDS; every pair has a wavefront (two from 65 sectors on) whose lanes own a shift each and
//                         walk its columns in order, four at a time where the sectors are a multiple of four -- no table of
//                         cosines, no lane without a sum to make.  The most pairs a microsecond
// The results come back through place_results_out, the only place that splits (distance, shift) into the callers' arrays.
#include <algorithm>
#include "lsa_place_io.h"
#include "lsa_wave.h"

using namespace lsa;

namespace
{
constexpr int kSearchThreads = 256;
constexpr int kShiftTile = 64;          // shifts whose cosines are in LDS at a time: one wavefront sums them
constexpr int kSearchBlocks = 2048;     // of a k_place_search launch, unless lsa_debug_set "place_max_blocks" says otherwise
constexpr int kRowsThreads = 256;
constexpr int kRowsWaves = kRowsThreads / 64;
constexpr int kRowsBlocks = 1024;      // of a k_place_search_rows launch, unless lsa_debug_set "place_max_blocks" says otherwise ...
constexpr int kRowsPiece = 32;         // ... or its pieces would be longer than this many tiles: then more workgroups
constexpr int kMaxLength = place::kMaxRings * place::kMaxSectors + place::kMaxSectors;
// k_place_search's LDS at the largest shape: two descriptors and a tile of cosines with rows of an odd length
static_assert((2 * kMaxLength + kShiftTile * (place::kMaxSectors | 1)) * sizeof(float) <= 64 * 1024, "k_place_search keeps to 64 KB of LDS");
// k_place_search_rows': the query and the candidates in flight -- four up to 64 sectors, two beyond
static_assert((1 + kRowsWaves) * (place::kMaxRings * 64 + 64) * sizeof(float) <= 64 * 1024, "k_place_search_rows keeps to 64 KB of LDS");
static_assert((1 + kRowsWaves / 2) * kMaxLength * sizeof(float) <= 64 * 1024, "k_place_search_rows keeps to 64 KB of LDS");

// the (distance, shift) arg-min's order for lsa_wave.h
struct Beats
{
  __device__ bool operator()(float d2, int s2, float d, int s) const { return place::beats(d2, s2, d, s); }
};

struct SearchArgs
{
  const float* slots;
  PlaceResult* out;     // [count]
  long long cap, head;  // the ring of slots
  int stride;
  int query, first, count;  // frames: the candidates are first .. first + count - 1
};

// A workgroup per candidate, striding over the range.  LDS: q and c whole (cells and norms), and the cosines of kShiftTile
// shifts, row = shift, rows of an odd length: the lanes that sum -- one per shift, each walking its row in column order, all
// at the same column -- then sit on distinct banks.  The cosines of a tile are spread over all lanes, column fastest, so
// q's reads are consecutive and c's consecutive up to the wrap.  A column that is empty in q or in c has no cosine; the
// summing lane tests the norms again rather than a marker in the table.  Lane s keeps the best of its shifts s, s + 64 (tiles
// ascending, so an equal distance never displaces the lower shift); the first wavefront reduces with the same rule.
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
        // (argmin_take's step written out: with the call the compiler lays the kernel out 1.2 % slower)
        const float d = place::shift_distance(sum, cnt, minCommon);
        if (bestShift < 0 || place::beats(d, s, best, bestShift)) { best = d; bestShift = s; }
      }
      __syncthreads();  // before the next tile overwrites the table
    }
    if (threadIdx.x < 64)
    {
      wave_argmin(best, bestShift, Beats());
      if (threadIdx.x == 0) a.out[b] = PlaceResult{best, bestShift};
    }
  }
}

template <bool kColumnTile>
__global__ __launch_bounds__(kRowsThreads) void k_place_search_rows(PlaceRun a, lsa_place_params_t p)
{
  extern __shared__ __align__(16) float s_lds[];
  __shared__ PlaceResult s_part[kRowsWaves];
  const int rings = p.rings, sectors = p.sectors, cells = rings * sectors, length = cells + sectors;
  const int minCommon = place::min_common(p);
  const int inFlight = place_pairs_in_flight(sectors), wpp = kRowsWaves / inFlight;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int slot = wave / wpp;                         // the pair of the tile this wavefront works on
  const int mine = (wave - slot * wpp) * 64 + lane;    // the thread among the pair's: its shift
  const int pairThreads = wpp * 64;
  const float* q = s_lds;
  float* c = s_lds + (size_t)length * (1 + slot);
  const float* nq = q + cells;
  const float* nc = c + cells;
  const long long t0 = (long long)blockIdx.x * a.tiles_per_block;
  const long long t1 = t0 + a.tiles_per_block < a.tiles ? t0 + a.tiles_per_block : a.tiles;
  if (t0 >= t1) return;
  int row = 0;
  for (int lo = 0, hi = a.nrows - 1; ; )  // the last row whose tiles begin at or before t0: the one t0 belongs to
  {
    if (lo >= hi) { row = lo; break; }
    const int mid = (lo + hi + 1) >> 1;
    if (a.rows[mid].tile0 <= t0) lo = mid;
    else hi = mid - 1;
  }
  int loaded = -1;
  for (long long t = t0; t < t1; ++t)
  {
    while (row + 1 < a.nrows && a.rows[row + 1].tile0 <= t) ++row;
    const PlaceRow r = a.rows[row];
    if (row != loaded)
    {
      // (the last tile's readers of q passed its second barrier)
      const float* __restrict__ src = a.slots + (size_t)((a.head + r.query) % a.cap) * (size_t)a.stride;
      for (int i = threadIdx.x; i < length; i += kRowsThreads) s_lds[i] = src[i];
      loaded = row;
    }
    const long long at = (t - r.tile0) * inFlight + slot;
    const bool inside = at < (long long)r.len;
    const int cand = inside ? (int)at : 0;
    bool compute = inside;
    if (compute && a.pos) compute = place::position_gate(a.pos[r.query], a.pos[cand], a.max_distance);
    if (compute)
    {
      const float* __restrict__ src = a.slots + (size_t)((a.head + cand) % a.cap) * (size_t)a.stride;
      for (int i = mine; i < length; i += pairThreads) c[i] = src[i];
    }
    __syncthreads();
    float best = 0.f;
    int bestShift = -1;
    if (compute && mine < sectors)
    {
      // PlaceDistance's loop for shift `mine`: the columns ascending, each cosine's dot over the rings ascending
      float sum = 0.f;
      int cnt = 0;
      if (kColumnTile && (sectors & 3) == 0)
      {
        // four columns at a time: q's four values are one 16-byte read, the same address for the whole wavefront; each of the
        // four dots adds its rings in order, and the cosines join the sum in the order of their columns (a dot nobody asks
        // for, its column empty on either side, is formed and dropped)
        for (int j0 = 0; j0 < sectors; j0 += 4)
        {
          int k[4];
          k[0] = mine + j0 >= sectors ? mine + j0 - sectors : mine + j0;
#pragma unroll
          for (int t = 1; t < 4; ++t) k[t] = k[t - 1] + 1 == sectors ? 0 : k[t - 1] + 1;
          float dot[4] = {0.f, 0.f, 0.f, 0.f};
          for (int ring = 0; ring < rings; ++ring)
          {
            const float4 qv = *reinterpret_cast<const float4*>(q + ring * sectors + j0);
            const float* cr = c + ring * sectors;
            dot[0] += qv.x * cr[k[0]];
            dot[1] += qv.y * cr[k[1]];
            dot[2] += qv.z * cr[k[2]];
            dot[3] += qv.w * cr[k[3]];
          }
#pragma unroll
          for (int t = 0; t < 4; ++t)
          {
            const float nqj = nq[j0 + t], nck = nc[k[t]];
            if (nqj > 0.f && nck > 0.f)
            {
              sum += dot[t] / (nqj * nck);  // place::cosine's quotient
              ++cnt;
            }
          }
        }
      }
      else
      {
        int k = mine;
        for (int j = 0; j < sectors; ++j)
        {
          const float nqj = nq[j], nck = nc[k];
          if (nqj > 0.f && nck > 0.f)
          {
            sum += place::cosine(q, c, rings, sectors, j, k, nqj, nck);
            ++cnt;
          }
          if (++k == sectors) k = 0;
        }
      }
      best = place::shift_distance(sum, cnt, minCommon);
      bestShift = mine;
    }
    wave_argmin(best, bestShift, Beats());
    if (lane == 0) s_part[wave] = PlaceResult{best, bestShift};
    __syncthreads();
    if (inside && mine == 0)
    {
      PlaceResult res = s_part[wave];
      if (wpp == 2) argmin_take(res.distance, res.shift, s_part[wave + 1].distance, s_part[wave + 1].shift, Beats());
      // a pair behind the position gate is not computed: its slot holds what no selection reads (a NaN has no rank)
      if (!compute) res = PlaceResult{__int_as_float(0x7fc00000), -1};
      a.table[r.offset + cand] = res;
    }
  }
}
}  // namespace

namespace lsa
{
void place_rows_launch(lsa_ctx* ctx, double bytes, PlaceRun a, const lsa_place_params_t& p)
{
  const size_t lds = (size_t)(1 + place_pairs_in_flight(p.sectors)) * place::length(p) * sizeof(float);  // <= 64 KB (the static_asserts above)
  // a workgroup's piece: tiles / 1 024, but no more than kRowsPiece tiles -- behind the position gate the work of a piece
  // varies from all of it to none, and pieces handed out as workgroups retire even that out ("place_max_blocks" n: n pieces)
  long long per = (a.tiles + kRowsBlocks - 1) / kRowsBlocks;
  if (per > kRowsPiece) per = kRowsPiece;
  if (ctx->place_max_blocks > 0) per = (a.tiles + ctx->place_max_blocks - 1) / ctx->place_max_blocks;
  const long long blocks = (a.tiles + per - 1) / per;
  a.tiles_per_block = per;
  ProfScope ps(ctx, "place_search_rows", bytes);
  if (ctx->place_untiled) hipLaunchKernelGGL(k_place_search_rows<false>, dim3((unsigned)blocks), dim3(kRowsThreads), lds, ctx->stream, a, p);
  else hipLaunchKernelGGL(k_place_search_rows<true>, dim3((unsigned)blocks), dim3(kRowsThreads), lds, ctx->stream, a, p);
}

int place_results_out(lsa_ctx* ctx, const PlaceResult* dev, PlaceResult* host, long long count, float* distance_out, int32_t* shift_out)
{
  LSA_HIP(ctx, hipMemcpyAsync(host, dev, (size_t)count * sizeof(PlaceResult), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (long long i = 0; i < count; ++i)
  {
    distance_out[i] = host[i].distance;
    shift_out[i] = host[i].shift;
  }
  return LSA_OK;
}

int place_search_one(lsa_ctx* ctx, const float* slots, long long cap, long long head, int stride, const lsa_place_params_t& p, int query, int first, int count,
                     float* distance_out, int32_t* shift_out)
{
  PlaceResults& res = ctx->place_results;
  const int rc = scratch_room(ctx, &res.dev, &res.pinned, &res.cap, (size_t)count);
  if (rc) return rc;
  const size_t lds = (size_t)(2 * place::length(p) + kShiftTile * (p.sectors | 1)) * sizeof(float);  // <= 64 KB (the static_assert above)
  const int blocks = std::min(count, ctx->place_max_blocks > 0 ? ctx->place_max_blocks : kSearchBlocks);
  SearchArgs a;
  a.slots = slots;
  a.out = res.dev;
  a.cap = cap;
  a.head = head;
  a.stride = stride;
  a.query = query;
  a.first = first;
  a.count = count;
  {
    ProfScope ps(ctx, "place_search", (double)(count + 1) * place::length(p) * 4 + (double)count * sizeof(PlaceResult));
    hipLaunchKernelGGL(k_place_search, dim3((unsigned)blocks), dim3(kSearchThreads), lds, ctx->stream, a, p);
  }
  LSA_HIP(ctx, hipGetLastError());
  return place_results_out(ctx, res.dev, res.pinned, count, distance_out, shift_out);
}
}  // namespace lsa
