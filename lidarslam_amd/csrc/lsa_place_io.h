// lsa_place_io.h -- what the table of map descriptors (lsa_map_place.hip) needs of the log's place unit (lsa_place.hip): its
// two kernels, launched on descriptors that live somewhere else.  A slot is rings * sectors + sectors floats either way.
#pragma once
#include <deque>
#include "lsa_ctx.h"

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
  void* table = nullptr;    // k_log_describe's frames
  size_t table_cap = 0;
  PlaceResult* result_dev = nullptr;
  PlaceResult* result_host = nullptr;  // pinned
  long long result_cap = 0;
  int described = 0;        // by the last call
  // loop detection: the ragged table of a run of queries; what a call uploads (positions, rows) and brings back (pinned twins)
  PlaceResult* rows_table = nullptr;
  long long rows_table_cap = 0;  // entries
  void* detect_up_dev = nullptr;
  void* detect_up_host = nullptr;
  size_t detect_up_cap = 0;      // bytes
  void* detect_res_dev = nullptr;
  void* detect_res_host = nullptr;
  size_t detect_res_cap = 0;     // bytes
};
// the argument check of the log's place calls, the store for these parameters, and a valid descriptor for every frame of
// first..last (one k_log_describe launch for those that had none; the store's `described` says how many)
int place_prepare(lsa_ctx* ctx, const char* who, const lsa_place_params_t* params, int first, int last);
// k_log_describe for `count` frames of a table in device memory: a workgroup per frame, slot f.slot of `slots`
void place_describe_launch(const DescribeFrame* frames_dev, int count, float* slots, int stride, const lsa_place_params_t& p, hipStream_t stream);
// k_place_search: slot (head + query) % cap against the slots (head + first + i) % cap, i < count -> out_dev[i]; a flat table
// is cap = its slots, head = 0
void place_search_launch(lsa_ctx* ctx, const float* slots, long long cap, long long head, int stride, int query, int first, int count, PlaceResult* out_dev,
                         const lsa_place_params_t& p, hipStream_t stream);
}  // namespace lsa
