// lsa_match_internal.h -- what the files of the matching step share on the host side: lsa_match.hip (C ABI),
// lsa_match_fused.hip (one launch per ICP iteration), lsa_match_staged.hip (staged cross-check), lsa_target.hip (search
// grids) and lsa_overlap.hip.
#pragma once
#include "lsa_knn.h"

namespace lsa
{

// one keypoint type's match, ready to be enqueued: parameters resolved, histogram block taken
struct MatchPrep
{
  int type;
  int ti;                       // target index (slot * 3 + type)
  const lsa_point_t* queries;
  int nq;
  MatchConst mc;
  float far_d2;                 // planes / blobs: the search may stop once the k-th neighbour is known to be farther
  int* hist;                    // device, 16 ints: [8] rejection histogram, [8], [9] hand-over counters
};

struct InterpConst;
InterpConst make_interp_const(const double H0[16], const double H1[16], double t0, double t1);  // lsa_transform.hip
// undistort: every keypoint is first moved by that motion interpolated at its own time, in place (lsa_undistort's step, folded
// into the search kernel); only when every keypoint of the set is among `preps` and is searched
// link >= 0: the launch waits behind that link (lsa_icp_link) and takes pose -- and, link_undistorts, the undistortion -- from it
int enqueue_fused_match(lsa_ctx* ctx, const MatchPrep* preps, int count, const double pose[16], hipStream_t st, const InterpConst* undistort = nullptr,
                        int link = -1, bool link_undistorts = false);
// lsa_match_staged.hip: one prepared match as the staged kernels; the exact kNN alone (k <= 5, 8, 16: three instantiations)
void enqueue_staged_match(lsa_ctx* ctx, const MatchPrep& mp, const double pose[16], hipStream_t st);
void enqueue_staged_knn(lsa_ctx* ctx, const lsa_point_t* q, int nq, const Rigid& pose, int k, float far_d2, int type, int ti, hipStream_t st, int* hist);
int flush_grids(lsa_ctx* ctx);                                              // lsa_target.hip: builds the grids of every target marked dirty
int next_hist_block(lsa_ctx* ctx, int type, hipStream_t st, int** hist);    // lsa_match.hip: the type's next block of the histogram ring

}  // namespace lsa
