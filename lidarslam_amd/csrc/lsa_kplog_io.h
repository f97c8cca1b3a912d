// lsa_kplog_io.h -- the keypoint log's replay of a RANGE of frames into destinations on the device (lsa_kplog.hip), for the
// library's own callers: the registration of logged frames (host/lsa_slam_log.cpp) replays the frames around a revisited
// pose into the batch buffers of scratch maps and the query frames into a keypoint set.  lsa_kplog_replay_range (the C ABI)
// is the same replay into pinned host memory.
#pragma once
#include "lsa_ctx.h"

namespace lsa
{
struct KpLogRange
{
  unsigned type_mask;
  const double* poses;  // n row-major 4x4: the poses of ALL logged frames
  const double* times;  // n
  int n;                // = lsa_kplog_size
  int first, last;      // the frames replayed, inclusive
  int rule;             // 0 rigid, 1 the rebuild's (t[i] - t[i-1], 0), 2 the sweep's (-(t[i] - t[i-1]), 0)
};
int kplog_replay_range_to_set(lsa_ctx* ctx, const KpLogRange& range, lsa_ctx* dst, int set, long long counts[3], float box_min[3][3], float box_max[3][3]);
int kplog_replay_range_to_grids(lsa_ctx* ctx, const KpLogRange& range, lsa_device_grid* const grids[3], bool fixed, double time, bool roll, long long counts[3],
                                float box_min[3][3], float box_max[3][3]);

// The log's frame table for its other unit, the descriptor store (lsa_place.hip): frame `frame`'s device pointers and counts.
// false: no such frame.
bool kplog_frame(const lsa_ctx* ctx, int frame, const lsa_point_t* pts[3], int n[3]);
// ... and what the log tells the store (each does nothing while there is no store)
void place_pop_front(lsa_ctx* ctx);
void place_clear(lsa_ctx* ctx);
void place_destroy(lsa_ctx* ctx);
}  // namespace lsa
