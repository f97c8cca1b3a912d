// lsa_place_io.h -- what the place units share: the log's descriptor store and k_log_describe (lsa_place.hip), the
// pair-distance kernels and the way their results come back (lsa_place_search.hip), loop detection (lsa_place_detect.hip)
// and the table of map descriptors (lsa_map_place.hip).  A slot is rings * sectors + sectors floats everywhere.
#pragma once
#include <cstring>
#include <deque>
#include <string>
#include "lsa_ctx.h"
#include "lsa_place_select.h"
#include "lsa_scan_descriptor.h"

namespace lsa
{
struct PlaceResult
{
  float distance;
  int shift;
};
// what k_log_describe turns into one slot
struct DescribeFrame
{
  const float4* pts[3];  // the frame's keypoints (a LidarPoint is two float4: x y z w, then the rest)
  int n[3];              // 0 for a type outside the mask
  int slot;
};
// the log's descriptor store (lsa_place.hip) and the scratch space of loop detection over it (lsa_place_detect.hip)
struct PlaceStore
{
  lsa_place_params_t params;
  bool have_params = false;
  float* slots = nullptr;
  long long cap = 0;        // slots
  int stride = 0;           // floats a slot
  long long head = 0;       // the slot of frame 0
  std::deque<char> valid;   // of the log's first valid.size() frames; the frames behind them have no descriptor
  char* table = nullptr;    // k_log_describe's frames
  size_t table_cap = 0;     // bytes
  int described = 0;        // by the last call
  // loop detection: the ragged table of a run of queries; what a call uploads (positions, rows) and brings back (pinned twins)
  PlaceResult* rows_table = nullptr;
  long long rows_table_cap = 0;  // entries
  char* detect_up_dev = nullptr;
  char* detect_up_host = nullptr;
  size_t detect_up_cap = 0;      // bytes
  char* detect_res_dev = nullptr;
  char* detect_res_host = nullptr;
  size_t detect_res_cap = 0;     // bytes
};

// the refusal of descriptor parameters out of limits, and whether two sets are the same one
inline int check_params(lsa_ctx* ctx, const char* who, const lsa_place_params_t* params)
{
  if (!params || !place::params_ok(*params)) return ctx->fail(LSA_E_ARG, std::string(who) + ": descriptor parameters out of limits");
  return LSA_OK;
}
inline bool same_params(const lsa_place_params_t& a, const lsa_place_params_t& b)
{
  static_assert(sizeof(lsa_place_params_t) == 4 * sizeof(int32_t) + 3 * sizeof(double), "no padding: compared by bytes");
  return std::memcmp(&a, &b, sizeof(a)) == 0;
}

// the argument check of the log's place calls, the store for these parameters, and a valid descriptor for every frame of
// first..last (one k_log_describe launch for those that had none; the store's `described` says how many)
int place_prepare(lsa_ctx* ctx, const char* who, const lsa_place_params_t* params, int first, int last);
// k_log_describe for `count` frames of a table in device memory: a workgroup per frame, slot f.slot of `slots`
void place_describe_launch(const DescribeFrame* frames_dev, int count, float* slots, int stride, const lsa_place_params_t& p, hipStream_t stream);

// ---- the pair-distance kernels (lsa_place_search.hip) ----------------------------------------------------------------------
// Descriptors live in a ring of slots, frame i in slot (head + i) % cap; a flat table is cap = its slots, head = 0.
// k_place_search: the frame `query` against the frames first .. first + count - 1 through the context's result buffers into
// the caller's arrays -- one launch under the ProfScope "place_search", one copy, one wait
int place_search_one(lsa_ctx* ctx, const float* slots, long long cap, long long head, int stride, const lsa_place_params_t& p, int query, int first, int count,
                     float* distance_out, int32_t* shift_out);
// a row of k_place_search_rows: query against the frames 0 .. len - 1 -> entries offset .. offset + len - 1 of the table;
// tile0: the first of its tiles among the run's (a tile: place_pairs_in_flight consecutive candidates of one row)
struct PlaceRow
{
  int query, len;
  long long offset, tile0;
};
LSA_HDP int place_pairs_in_flight(int sectors) { return sectors > 64 ? 2 : 4; }
struct PlaceRun
{
  const float* slots;
  long long cap, head;
  int stride;
  const PlaceRow* rows;  // on the device, ascending tile0
  int nrows;
  long long tiles, tiles_per_block;  // (the launcher's)
  PlaceResult* table;
  const place::FramePosition* pos;  // nullptr: no position gate; else a pair the gate refuses is not computed (NaN, -1)
  double max_distance;
};
// one launch on the context's stream under the ProfScope "place_search_rows"; lsa_debug_set "place_max_blocks" n: n pieces
void place_rows_launch(lsa_ctx* ctx, double bytes, PlaceRun run, const lsa_place_params_t& p);
// `count` results of device memory through `host` (pinned or not) into the caller's two arrays: one copy, one wait
int place_results_out(lsa_ctx* ctx, const PlaceResult* dev, PlaceResult* host, long long count, float* distance_out, int32_t* shift_out);
}  // namespace lsa
