// lsa_place_detect.hip -- loop detection over the whole keypoint log: many queries in one pass over the
// log's descriptor store (lsa_place.hip), the selection on the device too, only the candidates coming back.  The distance of
// two descriptors is lsa_scan_descriptor.h's, the gates and the ranking lsa_place_select.h's -- the texts the host statement
// (host/lsa_place.cpp: PlaceDetect) compiles; the kernels decide only who computes what.  The ragged table of a run of
// queries, row k = (distance, shift) of query q_k against the frames 0 .. len_k - 1, is k_place_search_rows'
// (lsa_place_search.hip); here are the plan of the runs and
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
#include "lsa_wave.h"

using namespace lsa;

namespace
{
constexpr int kSelectBlocks = 4096;    // of a select launch, unless lsa_debug_set "place_max_blocks" says otherwise
constexpr long long kTableBytes = 256ll << 20;  // the table's budget, unless lsa_debug_set "place_table_bytes" lowers it

struct DetectPick
{
  int frame, shift;
  float distance;
};

struct SelectArgs
{
  const PlaceRow* rows;
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
  const auto ranks_before = [](float d2, int i2, float d, int i) { return place::ranks_before(d2, i2, d, i); };
  for (int r = blockIdx.x; r < a.nrows; r += gridDim.x)
  {
    const PlaceRow row = a.rows[r];
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
        argmin_take(best, bestFrame, d, i, ranks_before);
      }
      wave_argmin(best, bestFrame, ranks_before);
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
  std::vector<PlaceRow> rows;      // of the call's queries, ascending
  std::vector<int> run_begin;       // the first row of every run, and the number of rows behind the last
  std::vector<long long> run_tiles, run_entries;
  long long max_entries = 0, computed_rows = 0;
};

// pos: the gates are on (len = the prefix the travelled gate admits); nullptr: every frame before the query
Plan make_plan(lsa_ctx* ctx, const lsa_loop_detect_t& d, int last, const place::FramePosition* pos)
{
  Plan plan;
  const int inFlight = place_pairs_in_flight(d.search.descriptor.sectors);
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
    plan.rows.push_back(PlaceRow{q, len, entries, tiles});
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

// the launch of a run over the log's store into the table, which has room for the plan's longest run
void search_run_launch(lsa_ctx* ctx, PlaceStore* st, const PlaceRow* rows_dev, const Plan& plan, size_t run, const place::FramePosition* pos_dev, double max_distance)
{
  PlaceRun a = {};
  a.slots = st->slots;
  a.cap = st->cap;
  a.head = st->head;
  a.stride = st->stride;
  a.rows = rows_dev + plan.run_begin[run];
  a.nrows = plan.run_begin[run + 1] - plan.run_begin[run];
  a.tiles = plan.run_tiles[run];
  a.table = st->rows_table;
  a.pos = pos_dev;
  a.max_distance = max_distance;
  place_rows_launch(ctx, (double)plan.run_entries[run] * (place::length(st->params) * 4. + sizeof(PlaceResult)), a, st->params);
}

// room for the plan's table, and for `up` bytes to go up and `res` to come back through pinned twins
int detect_room(lsa_ctx* ctx, PlaceStore* st, const Plan& plan, size_t up, size_t res)
{
  int rc = scratch_room<PlaceResult>(ctx, &st->rows_table, nullptr, &st->rows_table_cap, (size_t)plan.max_entries, 0, true);
  if (!rc) rc = scratch_room(ctx, &st->detect_up_dev, &st->detect_up_host, &st->detect_up_cap, up);
  if (!rc) rc = scratch_room(ctx, &st->detect_res_dev, &st->detect_res_host, &st->detect_res_cap, res);
  return rc;
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
  if (int rc = check_params(ctx, who, params)) return rc;
  if (!place::query_set_ok(lsa_kplog_size(ctx), first_query, last_query, query_stride, &last)) return refuse(ctx, who, "not a query set of the logged frames");
  if (!distance_out || !shift_out) return refuse(ctx, who, "bad argument");
  int rc = place_prepare(ctx, who, params, 0, last);
  if (rc) return rc;
  PlaceStore* st = ctx->place;
  const Plan plan = make_plan(ctx, d, last, nullptr);
  const size_t rows_bytes = plan.rows.size() * sizeof(PlaceRow);
  rc = detect_room(ctx, st, plan, rows_bytes, 0);
  if (rc) return rc;
  std::memcpy(st->detect_up_host, plan.rows.data(), rows_bytes);
  LSA_HIP(ctx, hipMemcpyAsync(st->detect_up_dev, st->detect_up_host, rows_bytes, hipMemcpyHostToDevice, ctx->stream));
  const PlaceRow* rows_dev = reinterpret_cast<const PlaceRow*>(st->detect_up_dev);
  std::vector<PlaceResult> back;
  size_t written = 0;
  for (size_t run = 0; run + 1 < plan.run_begin.size(); ++run)
  {
    const long long entries = plan.run_entries[run];
    if (entries == 0) continue;  // no pair, no launch
    search_run_launch(ctx, st, rows_dev, plan, run, nullptr, 0.);
    LSA_HIP(ctx, hipGetLastError());
    // (the whole table of a run, up to the budget: through pageable memory, nothing of that size is pinned for a debug call)
    back.resize((size_t)entries);
    rc = place_results_out(ctx, st->rows_table, back.data(), entries, distance_out + written, shift_out + written);
    if (rc) return rc;
    written += (size_t)entries;
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
  const size_t rows_bytes = plan.rows.size() * sizeof(PlaceRow);
  const size_t counts_bytes = ((size_t)queries * sizeof(int) + 15) / 16 * 16;
  const size_t res_bytes = counts_bytes + (size_t)queries * d.per_query * sizeof(DetectPick);
  rc = detect_room(ctx, st, plan, pos_bytes + rows_bytes, res_bytes);
  if (rc) return rc;
  std::memcpy(st->detect_up_host, pos.data(), pos_bytes);
  std::memcpy(st->detect_up_host + pos_bytes, plan.rows.data(), rows_bytes);
  LSA_HIP(ctx, hipMemcpyAsync(st->detect_up_dev, st->detect_up_host, pos_bytes + rows_bytes, hipMemcpyHostToDevice, ctx->stream));
  const place::FramePosition* pos_dev = reinterpret_cast<const place::FramePosition*>(st->detect_up_dev);
  const PlaceRow* rows_dev = reinterpret_cast<const PlaceRow*>(st->detect_up_dev + pos_bytes);
  int* counts_dev = reinterpret_cast<int*>(st->detect_res_dev);
  DetectPick* picks_dev = reinterpret_cast<DetectPick*>(st->detect_res_dev + counts_bytes);
  for (size_t run = 0; run + 1 < plan.run_begin.size(); ++run)
  {
    const int r0 = plan.run_begin[run], r1 = plan.run_begin[run + 1];
    if (plan.run_tiles[run] > 0)
    {
      search_run_launch(ctx, st, rows_dev, plan, run, d.search.max_distance > 0. ? pos_dev : nullptr, d.search.max_distance);
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
  const DetectPick* picks = reinterpret_cast<const DetectPick*>(st->detect_res_host + counts_bytes);
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
