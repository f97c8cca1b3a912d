// lsa_place_io.h -- what the table of map descriptors (lsa_map_place.hip) needs of the log's place unit (lsa_place.hip): its
// two kernels, launched on descriptors that live somewhere else.  A slot is rings * sectors + sectors floats either way.
#pragma once
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
// k_log_describe for `count` frames of a table in device memory: a workgroup per frame, slot f.slot of `slots`
void place_describe_launch(const DescribeFrame* frames_dev, int count, float* slots, int stride, const lsa_place_params_t& p, hipStream_t stream);
// k_place_search: slot (head + query) % cap against the slots (head + first + i) % cap, i < count -> out_dev[i]; a flat table
// is cap = its slots, head = 0
void place_search_launch(lsa_ctx* ctx, const float* slots, long long cap, long long head, int stride, int query, int first, int count, PlaceResult* out_dev,
                         const lsa_place_params_t& p, hipStream_t stream);
}  // namespace lsa
