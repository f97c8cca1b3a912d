// lsa_place_detect.hip -- loop detection over the whole keypoint log: many queries in one pass over the
// log's descriptor store (lsa_place.hip), the selection on the device too, only the candidates coming back.  The distance of
// two descriptors is lsa_scan_descriptor.h's, the gates and the ranking lsa_place_select.h's -- the texts the host statement
// (host/lsa_place.cpp: PlaceDetect) compiles; the kernels below decide only who computes what.
//   k_place_search_rows   the ragged table of a run of queries: row k = (distance, shift) of query q_k against the frames
//                         0 .. len_k - 1.  A workgroup walks a contiguous piece of the run's tiles (a tile: the pairs in flight,
//                         consecutive candidates of one query), so the query's descriptor stays in LDS; every pair has a
//                         wavefront (two from 65 sectors on) whose lanes own a shift each and walk its columns in order,
//                         four at a time where the sectors are a multiple of four -- no table of cosines, no lane without a
//                         sum to make
//   k_place_select_rows   a wavefront per query: up to per_query rounds of the arg-min under (distance, frame) over the row's
//                         entries that pass the gates and lie outside the window of every frame picked before
// A call: the positions and the rows go up once, a search and a select launch per run of queries whose tables fit the byte
// budget, the candidates accumulate on the device, one copy to pinned memory, one wait.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include "host/lsa_place.h"
#include "lsa_ctx.h"
#include "lsa_kplog_io.h"
#include "lsa_place_io.h"
#include "lsa_place_select.h"

using namespace lsa;

namespace
{
constexpr int kRowsThreads = 256;
constexpr int kRowsWaves = kRowsThreads / 64;
constexpr int kRowsBlocks = 1024;      // of a search launch, unless lsa_debug_set "place_max_blocks" says otherwise ...
constexpr int kRowsPiece = 32;         // ... or its pieces would be longer than this many tiles: then more workgroups
constexpr int kSelectBlocks = 4096;    // of a select launch, likewise
constexpr long long kTableBytes = 256ll << 20;  // the table's budget, unless lsa_debug_set "place_table_bytes" lowers it
constexpr int kMaxLength = place::kMaxRings * place::kMaxSectors + place::kMaxSectors;
// k_place_search_rows' LDS: the query and the candidates in flight -- four up to 64 sectors, two beyond
static_assert((1 + kRowsWaves) * (place::kMaxRings * 64 + 64) * sizeof(float) <= 64 * 1024, "k_place_search_rows keeps to 64 KB of LDS");
static_assert((1 + kRowsWaves / 2) * kMaxLength * sizeof(float) <= 64 * 1024, "k_place_search_rows keeps to 64 KB of LDS");

__host__ __device__ inline int waves_per_pair(int sectors) { return sectors > 64 ? 2 : 1; }

// a query of the run: its row of the table (entries from the run's first) and the first of its tiles (of the run's)
struct DetectRow
{
  int query, len;
  long long offset, tile0;
};
struct DetectPick
{
  int frame, shift;
  float distance;
};

struct RowsArgs
{
  const float* slots;
  long long cap, head;  // the store's ring
  int stride;
  const DetectRow* rows;
  int nrows;
  long long tiles, tiles_per_block;
  PlaceResult* table;
  const place::FramePosition* pos;  // nullptr: no position gate
  double max_distance;
};

template <bool kColumnTile>
__global__ __launch_bounds__(kRowsThreads) void k_place_search_rows(RowsArgs a, lsa_place_params_t p)
{
  extern __shared__ __align__(16) float s_lds[];
  __shared__ PlaceResult s_part[kRowsWaves];
  const int rings = p.rings, sectors = p.sectors, cells = rings * sectors, length = cells + sectors;
  const int minCommon = place::min_common(p);
  const int wpp = waves_per_pair(sectors), inFlight = kRowsWaves / wpp;
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
    const DetectRow r = a.rows[row];
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
    // the (distance, shift) arg-min is a total order: any tree gives the sequential loop's answer
    for (int off = 32; off > 0; off >>= 1)
    {
      const float d2 = __shfl_down(best, off);
      const int s2 = __shfl_down(bestShift, off);
      if (s2 >= 0 && (bestShift < 0 || place::beats(d2, s2, best, bestShift))) { best = d2; bestShift = s2; }
    }
    if (lane == 0) s_part[wave] = PlaceResult{best, bestShift};
    __syncthreads();
    if (inside && mine == 0)
    {
      PlaceResult res = s_part[wave];
      if (wpp == 2)
      {
        const PlaceResult o = s_part[wave + 1];
        if (o.shift >= 0 && (res.shift < 0 || place::beats(o.distance, o.shift, res.distance, res.shift))) res = o;
      }
      // a pair behind the position gate is not computed: its slot holds what no selection reads (a NaN has no rank)
      if (!compute) res = PlaceResult{__int_as_float(0x7fc00000), -1};
      a.table[r.offset + cand] = res;
    }
  }
}

struct SelectArgs
{
  const DetectRow* rows;
  int nrows;
  const PlaceResult* table;
  const place::FramePosition* pos;
  double max_distance, max_descriptor_distance;
  int half_window, per_query;
  int* counts;        // of the run's queries
  DetectPick* picks;  // per_query a query
};

// A wavefront per query.  The picked frames stay in registers (the loops over them are unrolled over kMaxPerQuery).
__global__ __launch_bounds__(64) void k_place_select_rows(SelectArgs a)
{
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < a.nrows; r += gridDim.x)
  {
    const DetectRow row = a.rows[r];
    const PlaceResult* __restrict__ e = a.table + row.offset;
    const place::FramePosition pq = a.pos[row.query];
    int picked[place::kMaxPerQuery];
#pragma unroll
    for (int k = 0; k < place::kMaxPerQuery; ++k) picked[k] = 0;
    int found = 0;
    while (found < a.per_query)
    {
      float best = 0.f;
      int bestFrame = -1;
      for (int i = lane; i < row.len; i += 64)
      {
        const float d = e[i].distance;
        if (!place::descriptor_gate(d, a.max_descriptor_distance)) continue;
        bool out = false;
#pragma unroll
        for (int k = 0; k < place::kMaxPerQuery; ++k)
          if (k < found && place::excluded_by(i, picked[k], a.half_window)) out = true;
        if (out) continue;
        if (!place::position_gate(pq, a.pos[i], a.max_distance)) continue;
        if (bestFrame < 0 || place::ranks_before(d, i, best, bestFrame)) { best = d; bestFrame = i; }
      }
      for (int off = 32; off > 0; off >>= 1)
      {
        const float d2 = __shfl_down(best, off);
        const int i2 = __shfl_down(bestFrame, off);
        if (i2 >= 0 && (bestFrame < 0 || place::ranks_before(d2, i2, best, bestFrame))) { best = d2; bestFrame = i2; }
      }
      best = __shfl(best, 0);
      bestFrame = __shfl(bestFrame, 0);
      if (bestFrame < 0) break;
      if (lane == 0) a.picks[(size_t)r * a.per_query + found] = DetectPick{bestFrame, e[bestFrame].shift, best};
#pragma unroll
      for (int k = 0; k < place::kMaxPerQuery; ++k)
        if (k == found) picked[k] = bestFrame;
      ++found;
    }
    if (lane == 0) a.counts[r] = found;
  }
}

// ---- the host's side -----------------------------------------------------------------------------------------------------------
struct Plan
{
  std::vector<DetectRow> rows;      // of the call's queries, ascending
  std::vector<int> run_begin;       // the first row of every run, and the number of rows behind the last
  std::vector<long long> run_tiles, run_entries;
  long long max_entries = 0, computed_rows = 0;
};

// pos: the gates are on (len = the prefix the travelled gate admits); nullptr: every frame before the query
Plan make_plan(lsa_ctx* ctx, const lsa_loop_detect_t& d, int last, const place::FramePosition* pos)
{
  Plan plan;
  const int inFlight = kRowsWaves / waves_per_pair(d.search.descriptor.sectors);
  long long budget = (ctx->place_table_bytes > 0 ? (long long)ctx->place_table_bytes : kTableBytes) / (long long)sizeof(PlaceResult);
  if (budget < 1) budget = 1;
  long long entries = 0, tiles = 0;
  for (int q = d.first_query;; q += d.query_stride)
  {
    int len = q;
    if (pos)
    {
      int lo = 0, hi = q;  // the frames that pass are a prefix (lsa_place_select.h): its length
      while (lo < hi)
      {
        const int mid = lo + (hi - lo) / 2;
        if (place::travelled_gate(pos[q], pos[mid], d.search.min_travelled)) lo = mid + 1;
        else hi = mid;
      }
      len = lo;
    }
    if (plan.run_begin.empty() || (entries > 0 && entries + len > budget))
    {
      if (!plan.run_begin.empty()) { plan.run_entries.push_back(entries); plan.run_tiles.push_back(tiles); }
      plan.run_begin.push_back((int)plan.rows.size());
      entries = tiles = 0;
    }
    plan.rows.push_back(DetectRow{q, len, entries, tiles});
    entries += len;
    tiles += (len + inFlight - 1) / inFlight;
    plan.max_entries = std::max(plan.max_entries, entries);
    if (q > last - d.query_stride) break;  // (q + stride may not be an int)
  }
  plan.run_entries.push_back(entries);
  plan.run_tiles.push_back(tiles);
  plan.run_begin.push_back((int)plan.rows.size());
  return plan;
}

int grow(lsa_ctx* ctx, void** dev, void** host, size_t* cap, size_t bytes)
{
  if (bytes <= *cap) return LSA_OK;
  retire_dev(ctx, *dev);
  if (host) retire_host(ctx, *host);
  *dev = nullptr;
  if (host) *host = nullptr;
  *cap = 0;
  const size_t want = bytes + bytes / 2;
  LSA_HIP(ctx, hipMalloc(dev, want));
  if (host) LSA_HIP(ctx, hipHostMalloc(host, want, hipHostMallocDefault));
  *cap = want;
  return LSA_OK;
}

int ensure_table(lsa_ctx* ctx, PlaceStore* st, long long entries)
{
  if (entries <= st->rows_table_cap) return LSA_OK;
  retire_dev(ctx, st->rows_table);
  st->rows_table = nullptr;
  st->rows_table_cap = 0;
  LSA_HIP(ctx, hipMalloc((void**)&st->rows_table, (size_t)entries * sizeof(PlaceResult)));
  st->rows_table_cap = entries;
  return LSA_OK;
}

void search_rows_launch(lsa_ctx* ctx, PlaceStore* st, const DetectRow* rows_dev, int nrows, long long tiles, long long entries, const place::FramePosition* pos_dev,
                        double max_distance)
{
  const lsa_place_params_t& p = st->params;
  const int inFlight = kRowsWaves / waves_per_pair(p.sectors);
  const size_t lds = (size_t)(1 + inFlight) * place::length(p) * sizeof(float);  // <= 64 KB (the static_asserts above)
  // a workgroup's piece: tiles / 1 024, but no more than kRowsPiece tiles -- behind the position gate the work of a piece
  // varies from all of it to none, and pieces handed out as workgroups retire even that out ("place_max_blocks" n: n pieces)
  long long per = (tiles + kRowsBlocks - 1) / kRowsBlocks;
  if (per > kRowsPiece) per = kRowsPiece;
  if (ctx->place_max_blocks > 0) per = (tiles + ctx->place_max_blocks - 1) / ctx->place_max_blocks;
  const long long blocks = (tiles + per - 1) / per;
  RowsArgs a;
  a.slots = st->slots;
  a.cap = st->cap;
  a.head = st->head;
  a.stride = st->stride;
  a.rows = rows_dev;
  a.nrows = nrows;
  a.tiles = tiles;
  a.tiles_per_block = per;
  a.table = st->rows_table;
  a.pos = pos_dev;
  a.max_distance = max_distance;
  ProfScope ps(ctx, "place_search_rows", (double)entries * (place::length(p) * 4. + sizeof(PlaceResult)));
  if (ctx->place_untiled) hipLaunchKernelGGL(k_place_search_rows<false>, dim3((unsigned)blocks), dim3(kRowsThreads), lds, ctx->stream, a, p);
  else hipLaunchKernelGGL(k_place_search_rows<true>, dim3((unsigned)blocks), dim3(kRowsThreads), lds, ctx->stream, a, p);
}

int refuse(lsa_ctx* ctx, const char* who, const char* what) { return ctx->fail(LSA_E_ARG, std::string(who) + ": " + what); }
}  // namespace

extern "C" {

int lsa_kplog_place_search_rows(lsa_ctx* ctx, const lsa_place_params_t* params, int first_query, int last_query, int query_stride, float* distance_out,
                                int32_t* shift_out)
{
  const char* who = "lsa_kplog_place_search_rows";
  if (!ctx) return LSA_E_ARG;
  lsa_loop_detect_t d;
  lsa_loop_detect_init(&d);
  if (params) d.search.descriptor = *params;
  d.first_query = first_query;
  d.last_query = last_query;
  d.query_stride = query_stride;
  int last = 0;
  if (!params || !place::params_ok(*params)) return refuse(ctx, who, "descriptor parameters out of limits");
  if (!place::query_set_ok(lsa_kplog_size(ctx), first_query, last_query, query_stride, &last)) return refuse(ctx, who, "not a query set of the logged frames");
  if (!distance_out || !shift_out) return refuse(ctx, who, "bad argument");
  int rc = place_prepare(ctx, who, params, 0, last);
  if (rc) return rc;
  PlaceStore* st = ctx->place;
  const Plan plan = make_plan(ctx, d, last, nullptr);
  rc = ensure_table(ctx, st, plan.max_entries);
  if (rc) return rc;
  const size_t rows_bytes = plan.rows.size() * sizeof(DetectRow);
  rc = grow(ctx, &st->detect_up_dev, &st->detect_up_host, &st->detect_up_cap, rows_bytes);
  if (rc) return rc;
  std::memcpy(st->detect_up_host, plan.rows.data(), rows_bytes);
  LSA_HIP(ctx, hipMemcpyAsync(st->detect_up_dev, st->detect_up_host, rows_bytes, hipMemcpyHostToDevice, ctx->stream));
  const DetectRow* rows_dev = reinterpret_cast<const DetectRow*>(st->detect_up_dev);
  std::vector<PlaceResult> back;
  size_t written = 0;
  for (size_t run = 0; run + 1 < plan.run_begin.size(); ++run)
  {
    const long long entries = plan.run_entries[run];
    if (entries == 0) continue;  // no pair, no launch
    const int r0 = plan.run_begin[run], r1 = plan.run_begin[run + 1];
    search_rows_launch(ctx, st, rows_dev + r0, r1 - r0, plan.run_tiles[run], entries, nullptr, 0.);
    LSA_HIP(ctx, hipGetLastError());
    back.resize((size_t)entries);
    LSA_HIP(ctx, hipMemcpyAsync(back.data(), st->rows_table, (size_t)entries * sizeof(PlaceResult), hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (long long i = 0; i < entries; ++i, ++written)
    {
      distance_out[written] = back[(size_t)i].distance;
      shift_out[written] = back[(size_t)i].shift;
    }
  }
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return LSA_OK;
}

int lsa_kplog_detect_loops(lsa_ctx* ctx, const lsa_loop_detect_t* detect, const double* poses17, int n, lsa_loop_candidate_t* out, int capacity)
{
  const char* who = "lsa_kplog_detect_loops";
  if (!ctx) return LSA_E_ARG;
  lsa_loop_detect_t d;
  lsa_loop_detect_init(&d);
  if (detect) d = *detect;
  if (!poses17 || n != lsa_kplog_size(ctx)) return refuse(ctx, who, "as many poses as logged frames");
  int last = 0;
  const int queries = host::DetectQueries(d, n, capacity, &last);
  if (queries < 0) return refuse(ctx, who, "a query set outside the log, per_query outside 1..16, room for fewer than queries * per_query candidates, or parameters out of limits");
  if (!out) return refuse(ctx, who, "no place for the candidates");
  int rc = place_prepare(ctx, who, &d.search.descriptor, 0, last);
  if (rc) return rc;
  PlaceStore* st = ctx->place;
  // what goes up: the positions with travelled[] as PlaceSelect sums it, then the rows; what comes back: counts, then picks
  const size_t pos_bytes = (size_t)n * sizeof(place::FramePosition);
  std::vector<place::FramePosition> pos((size_t)n);
  host::FramePositions(poses17, n, pos.data());
  const Plan plan = make_plan(ctx, d, last, pos.data());
  const size_t rows_bytes = plan.rows.size() * sizeof(DetectRow);
  const size_t counts_bytes = ((size_t)queries * sizeof(int) + 15) / 16 * 16;
  const size_t res_bytes = counts_bytes + (size_t)queries * d.per_query * sizeof(DetectPick);
  rc = ensure_table(ctx, st, plan.max_entries);
  if (rc) return rc;
  rc = grow(ctx, &st->detect_up_dev, &st->detect_up_host, &st->detect_up_cap, pos_bytes + rows_bytes);
  if (rc) return rc;
  rc = grow(ctx, &st->detect_res_dev, &st->detect_res_host, &st->detect_res_cap, res_bytes);
  if (rc) return rc;
  std::memcpy(st->detect_up_host, pos.data(), pos_bytes);
  std::memcpy(static_cast<char*>(st->detect_up_host) + pos_bytes, plan.rows.data(), rows_bytes);
  LSA_HIP(ctx, hipMemcpyAsync(st->detect_up_dev, st->detect_up_host, pos_bytes + rows_bytes, hipMemcpyHostToDevice, ctx->stream));
  const place::FramePosition* pos_dev = reinterpret_cast<const place::FramePosition*>(st->detect_up_dev);
  const DetectRow* rows_dev = reinterpret_cast<const DetectRow*>(static_cast<char*>(st->detect_up_dev) + pos_bytes);
  int* counts_dev = reinterpret_cast<int*>(st->detect_res_dev);
  DetectPick* picks_dev = reinterpret_cast<DetectPick*>(static_cast<char*>(st->detect_res_dev) + counts_bytes);
  for (size_t run = 0; run + 1 < plan.run_begin.size(); ++run)
  {
    const int r0 = plan.run_begin[run], r1 = plan.run_begin[run + 1];
    if (plan.run_tiles[run] > 0)
    {
      search_rows_launch(ctx, st, rows_dev + r0, r1 - r0, plan.run_tiles[run], plan.run_entries[run], d.search.max_distance > 0. ? pos_dev : nullptr, d.search.max_distance);
      LSA_HIP(ctx, hipGetLastError());
    }
    SelectArgs a;
    a.rows = rows_dev + r0;
    a.nrows = r1 - r0;
    a.table = st->rows_table;
    a.pos = pos_dev;
    a.max_distance = d.search.max_distance;
    a.max_descriptor_distance = d.search.max_descriptor_distance;
    a.half_window = d.search.exclusion_half_window;
    a.per_query = d.per_query;
    a.counts = counts_dev + r0;
    a.picks = picks_dev + (size_t)r0 * d.per_query;
    const int blocks = std::min(r1 - r0, ctx->place_max_blocks > 0 ? ctx->place_max_blocks : kSelectBlocks);
    {
      ProfScope ps(ctx, "place_select_rows", (double)plan.run_entries[run] * sizeof(PlaceResult));
      hipLaunchKernelGGL(k_place_select_rows, dim3((unsigned)blocks), dim3(64), 0, ctx->stream, a);
    }
    LSA_HIP(ctx, hipGetLastError());
  }
  LSA_HIP(ctx, hipMemcpyAsync(st->detect_res_host, st->detect_res_dev, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int* counts = reinterpret_cast<const int*>(st->detect_res_host);
  const DetectPick* picks = reinterpret_cast<const DetectPick*>(static_cast<const char*>(st->detect_res_host) + counts_bytes);
  int found = 0;
  for (int k = 0; k < queries; ++k)
    for (int j = 0; j < counts[k]; ++j)
    {
      const DetectPick& pk = picks[(size_t)k * d.per_query + j];
      lsa_loop_candidate_t c;
      std::memset(&c, 0, sizeof(c));
      c.query = plan.rows[(size_t)k].query;
      c.frame = pk.frame;
      c.shift = pk.shift;
      c.distance = pk.distance;
      c.yaw = place::yaw_of(pk.shift, d.search.descriptor.sectors);
      out[found++] = c;
    }
  return found;
}

}  // extern "C"
