// lsa_match_staged.hip -- the staged exact kNN search and its model kernel: KDTreePCLAdaptor::KnnSearch
// (slam_lib/include/LidarSlam/KDTreePCLAdaptor.h:79-105) and KeypointsMatcher::BuildLineMatch / BuildPlaneMatch /
// BuildBlobMatch (slam_lib/src/KeypointsMatcher.cxx:106-346) as three launches per keypoint type.  Production matches
// with the one-launch form of lsa_match_fused.hip; this path is the cross-check (lsa_set_fused_match(ctx, 0)) and the
// 1-NN search of the overlap estimator (lsa_overlap.hip).  Both search the grids of lsa_target.hip.
//   k_knn_first /   EXACT k-nearest neighbours.  G lanes per query
//   k_knn_second    search the 3x3x3, then the 5x5x5 block of cells around it; a block's rows are contiguous
//                   runs of the cell-sorted array, flattened by a group prefix sum and dealt evenly to the
//                   lanes; the k best are picked by k rounds of group-minimum (DPP), identical instructions in
//                   every lane.  A round settles the query when k picks lie inside the radius the block
//                   proves; the few percent left go, through a device list, to the second kernel (one
//                   wavefront each, coarser levels, finally the whole target).
//   k_model<..>     one thread per keypoint: neighbourhood
//                   filter (per-ring :349-405 / RANSAC line :408-480, candidates staged in LDS), PCA in
//                   double, validity tests, residual record (A, P, X, weight)
// kNN order: ascending (float squared distance, target index); the distance is evaluated exactly like
// nanoflann's L2_Simple_Adaptor: ((dx*dx)+dy*dy)+dz*dz with d = query - point.
#include <cmath>
#include <type_traits>
#include "lsa_ctx.h"
#include "lsa_device_math.h"
#include "lsa_knn.h"
#include "lsa_match_internal.h"

using namespace lsa;

namespace
{

// Selection-based search (k_knn_first / k_knn_second).  G lanes cooperate on one query.  The rows of the
// block of cells being searched are contiguous runs of the cell-sorted array; their bounds are fetched by
// as many lanes at once, flattened with a group prefix sum, and the candidates are dealt to the lanes evenly,
// U per lane and batch, all loads in flight together.  The k best of (previous best + batch) are then PICKED:
// k rounds of "group minimum by (distance, index), owner retires it".  Every lane executes the same
// instructions whatever its candidates are -- no per-lane sorted lists, no divergent insertion, no merge
// tree -- and the result sits in registers that are uniform across the group.
template <int KMAX, int G, int U>
struct GroupSelect
{
  static constexpr int C = (KMAX + G - 1) / G;  // carry slots per lane: the previous best, dealt over the group
  knn_key key[U + C];   // [0, U) fresh candidates of the batch, [U, U + C) carry
  knn_key best[KMAX];   // ascending, uniform across the group; kKeyEmpty = none
  __device__ __forceinline__ void reset()
  {
#pragma unroll
    for (int s = 0; s < KMAX; ++s) best[s] = kKeyEmpty;
#pragma unroll
    for (int u = 0; u < U + C; ++u) key[u] = kKeyEmpty;
  }
  // best <- the k smallest of (carry slots + the fresh candidates of every lane); nfresh: fresh slots any group
  // of the wavefront uses in this batch (wave-uniform; the others hold nothing and are not looked at)
  __device__ __forceinline__ void select(int k, int gl, int nfresh)
  {
    // nothing in this batch beats the current k-th best of any group of the wavefront: keep the list
    knn_key kth = kKeyEmpty;
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
      if (s == k - 1) kth = best[s];
    bool improves = false;
#pragma unroll
    for (int u = 0; u < U; ++u) improves |= key[u] < kth;
    if (!__any(improves)) return;
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
    {
      if (s < k)
      {
        knn_key m = key[U];
#pragma unroll
        for (int c = 1; c < C; ++c) m = key[U + c] < m ? key[U + c] : m;
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (u < nfresh) m = key[u] < m ? key[u] : m;
        group_min<G>(m);
        best[s] = m;
        // the owner retires it (keys of real candidates are unique; empty slots all look alike, harmless)
#pragma unroll
        for (int c = 0; c < C; ++c)
          if (key[U + c] == m) key[U + c] = kKeyEmpty;
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (u < nfresh && key[u] == m) key[u] = kKeyEmpty;
      }
    }
    // the new best becomes the carry of the next batch: entry s lives in slot s / G of lane s % G
#pragma unroll
    for (int c = 0; c < C; ++c) key[U + c] = kKeyEmpty;
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
      if (s < k && gl == s % G) key[U + s / G] = best[s];
  }
  __device__ __forceinline__ int count_below(float bound2, int k) const
  {
    int c = 0;
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
      if (s < k && key_d2(best[s]) < bound2) ++c;
    return c;
  }
};

// the rows of one block of cells, dealt E per lane and flattened: candidate c of [0, total) is an offset into
// the cell-sorted array
template <int G, int E>
struct BlockRuns
{
  static constexpr int kE = E;
  uint32_t b[E], len[E];
  uint32_t excl, total;
  bool covered;
  // every lane of the wavefront calls these (shuffles); groups with live == false get an empty block.
  // fetch() only issues the loads of the row bounds, finish() consumes them: several blocks can be fetched
  // before the first is finished, their loads overlap.
  __device__ __forceinline__ void fetch(const GridView& gv, int r, int gl, bool live)
  {
    const int nx = gv.g.dims[0], ny = gv.g.dims[1], nz = gv.g.dims[2];
    const int z0 = max(0, gv.cz - r), z1 = min(nz - 1, gv.cz + r);
    const int y0 = max(0, gv.cy - r), y1 = min(ny - 1, gv.cy + r);
    const int x0 = max(0, gv.cx - r), x1 = min(nx - 1, gv.cx + r);
    const int ys = y1 - y0 + 1;
    const int nrows = live ? (z1 - z0 + 1) * ys : 0;
    covered = (x0 == 0 && y0 == 0 && z0 == 0 && x1 == nx - 1 && y1 == ny - 1 && z1 == nz - 1);
    const int inv_ys = (1 << 16) / ys + 1;  // ri / ys == (ri * inv_ys) >> 16 for ys <= 9, ri < 128: no integer division in the loop
#pragma unroll
    for (int e = 0; e < E; ++e)
    {
      const int ri = gl * E + e;
      b[e] = 0; len[e] = 0;
      if (ri < nrows)
      {
        const int zi = (ri * inv_ys) >> 16;
        const int row = ((z0 + zi) * ny + (y0 + ri - zi * ys)) * nx;
        b[e] = gv.cell_start[row + x0];
        len[e] = gv.cell_start[row + x1 + 1];  // end of the run until finish()
      }
    }
  }
  __device__ __forceinline__ void finish(int gl)
  {
    uint32_t mine = 0;
#pragma unroll
    for (int e = 0; e < E; ++e)
    {
      len[e] -= b[e];
      mine += len[e];
    }
    uint32_t inc = mine;
#pragma unroll
    for (int o = 1; o < G; o <<= 1)
    {
      const uint32_t t = __shfl_up(inc, o, G);
      if (gl >= o) inc += t;
    }
    excl = inc - mine;  // non-decreasing over the lanes of the group
    total = __shfl(inc, G - 1, G);
  }
  __device__ __forceinline__ void build(const GridView& gv, int r, int gl, bool live)
  {
    fetch(gv, r, gl, live);
    finish(gl);
  }
  // the whole target as one run (exhaustive stage)
  __device__ __forceinline__ void whole(uint32_t m, int gl)
  {
#pragma unroll
    for (int e = 0; e < E; ++e) { b[e] = 0; len[e] = 0; }
    if (gl == 0) len[0] = m;
    excl = gl == 0 ? 0u : m;
    total = m;
    covered = true;
  }
  __device__ __forceinline__ uint32_t locate(uint32_t c) const
  {
    // the last lane L of the group with excl[L] <= c owns candidate c (then c < excl[L + 1]: it has a non-empty row)
    int L = 0;
#pragma unroll
    for (int step = G / 2; step > 0; step >>= 1)
    {
      const uint32_t ex = __shfl(excl, L + step, G);
      if (ex <= c) L += step;
    }
    uint32_t off = c - __shfl(excl, L, G);
    if constexpr (E == 1) return __shfl(b[0], L, G) + off;  // the lane's only row holds it
    uint32_t addr = 0;
    bool found = false;
#pragma unroll
    for (int e = 0; e < E; ++e)
    {
      const uint32_t bb = __shfl(b[e], L, G), ll = __shfl(len[e], L, G);
      if (!found && off < ll) { addr = bb + off; found = true; }
      if (!found) off -= ll;
    }
    return addr;
  }
};

// one search round: the k best of the block's candidates end up in sel.best (uniform across the group)
template <int KMAX, int G, int U, int E>
__device__ __forceinline__ void search_block(GroupSelect<KMAX, G, U>& sel, const BlockRuns<G, E>& runs, const float4* __restrict__ sorted, int k, int gl,
                                             float qx, float qy, float qz)
{
  sel.reset();
  // software pipeline: the loads of batch i + 1 are in flight while batch i is being picked from
  float4 nxt[U];
  auto issue = [&](uint32_t base) {
#pragma unroll
    for (int u = 0; u < U; ++u)
    {
      // a slot no group of the wavefront has a candidate for costs nothing (most blocks fill one or two slots)
      if (!__any(base + u * G + gl < runs.total)) break;
      const uint32_t c = base + u * G + gl;
      const uint32_t addr = runs.locate(c);
      nxt[u] = sorted[c < runs.total ? addr : 0];
    }
  };
  if (__any(0u < runs.total)) issue(0);
  for (uint32_t base = 0; __any(base < runs.total); base += G * U)
  {
    float4 p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) p[u] = nxt[u];
    if (__any(base + G * U < runs.total)) issue(base + G * U);
    int nfresh = 0;
#pragma unroll
    for (int u = 0; u < U; ++u)
    {
      const bool ok = base + u * G + gl < runs.total;
      if (__any(ok)) nfresh = u + 1;
      const float dx = qx - p[u].x, dy = qy - p[u].y, dz = qz - p[u].z;
      sel.key[u] = ok ? make_key((dx * dx + dy * dy) + dz * dz, __float_as_int(p[u].w)) : kKeyEmpty;
    }
    sel.select(k, gl, nfresh);
  }
}

// First stage: every query, G lanes each, the 3x3x3, then the 5x5x5 (and with RMAX = 3 the 7x7x7) block of the
// finest grid (each round searches its whole block afresh: no bookkeeping of what the previous round saw).
// Queries that are not settled inside RMAX cells go to the second stage through the device list.
template <int KMAX, int G, int RMAX>
__global__ __launch_bounds__(256) void k_knn_first(const float4* __restrict__ queries, int nq, Rigid pose, int k, float far_d2,
                                                   const GridDesc* __restrict__ desc, GridPtrs gp, int* __restrict__ knn_idx,
                                                   float* __restrict__ knn_d2, int* __restrict__ knn_cnt, int cap, int* __restrict__ count_out,
                                                   int* __restrict__ list_out, float4* __restrict__ list_pts)
{
  constexpr int U = 4;
  const int gl = threadIdx.x % G;
  const int q = (int)(((size_t)blockIdx.x * 256 + threadIdx.x) / G);
  const bool active = q < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (active)
  {
    // KeypointsMatcher: worldPoint = PosePrior * basePoint in double, narrowed to float for the search
    const float4 q4 = queries[2 * (size_t)q];
    double wx, wy, wz;
    rigid_apply(pose, (double)q4.x, (double)q4.y, (double)q4.z, wx, wy, wz);
    qx = (float)wx; qy = (float)wy; qz = (float)wz;
  }
  GridView gv;
  grid_view(gv, desc, gp.cell_start[0], gp.sorted[0], qx, qy, qz);
  GroupSelect<KMAX, G, U> sel;
  sel.reset();
  bool done = !active, far = false, deferred = false;
  // the row bounds of every round's block in one memory round trip (a later round costs one trip less); each
  // block has its own number of rows per lane, so that locating a candidate in the 3x3x3 block costs no more
  // shuffles than its 9 rows need
  constexpr int E1 = (9 + G - 1) / G, E2 = (25 + G - 1) / G, E3 = (49 + G - 1) / G;
  BlockRuns<G, E1> runs1;
  BlockRuns<G, E2> runs2;
  BlockRuns<G, (RMAX >= 3 ? E3 : 1)> runs3;
  runs1.fetch(gv, 1, gl, active);
  runs2.fetch(gv, 2, gl, active);
  if (RMAX >= 3) runs3.fetch(gv, 3, gl, active);
  auto round = [&](auto& runs, int r) {
    if (__all(done)) return;
    runs.finish(gl);
    if (done) runs.total = 0;  // groups that are done keep their result: an empty block, `cur` is scratch for them
    GroupSelect<KMAX, G, U> cur;
    search_block<KMAX, G, U, std::remove_reference_t<decltype(runs)>::kE>(cur, runs, gv.sorted, k, gl, qx, qy, qz);
    if (done) return;
    sel = cur;
    // every point closer than r cells (minus a 0.1 % guard for the float cell assignment) has been seen
    const float br = ((float)r - 0.001f) * gv.g.cell;
    const float bound2 = gv.outd2 + br * br;
    if (runs.covered || sel.count_below(bound2, k) >= k) done = true;
    else if (bound2 > far_d2) { far = true; done = true; }
    else if (r == RMAX)
    {
      // handed to the second stage: the query in target coordinates, and an upper bound of the k-th distance
      // (the k-th best seen so far; +inf when the block holds fewer than k points)
      if (gl == 0)
      {
        float ub = INFINITY;
#pragma unroll
        for (int s = 0; s < KMAX; ++s)
          if (s == k - 1) ub = key_d2(sel.best[s]);
        const int slot = atomicAdd(count_out, 1);
        list_out[slot] = q;
        list_pts[slot] = make_float4(qx, qy, qz, ub);
      }
      deferred = true;
      done = true;
    }
  };
  round(runs1, 1);
  round(runs2, 2);
  if (RMAX >= 3) round(runs3, 3);
  if (active && gl == 0 && !deferred)
  {
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < KMAX; ++s)
      if (s < k)
      {
        knn_idx[(size_t)s * cap + q] = key_idx(sel.best[s]);
        knn_d2[(size_t)s * cap + q] = key_d2(sel.best[s]);
        if (sel.best[s] != kKeyEmpty) ++cnt;
      }
    knn_cnt[q] = far ? kKnnFar : cnt;
  }
}

// Second and last stage: one wavefront per query the first stage handed over (a few percent: the isolated
// keypoints).  Coarser levels, blocks of 3^3, 5^3, 7^3 cells each, finally the whole target as one
// run, so every query leaves this kernel answered.  Same (distance, index) order everywhere => the result
// does not depend on the route taken.
template <int KMAX>
__global__ __launch_bounds__(256) void k_knn_second(const int* __restrict__ list_in, const float4* __restrict__ list_pts, const int* __restrict__ count_in,
                                                    int list_cap, int k, float far_d2, const GridDesc* __restrict__ desc, GridPtrs gp,
                                                    int* __restrict__ knn_idx, float* __restrict__ knn_d2, int* __restrict__ knn_cnt, int cap,
                                                    int* __restrict__ exhaustive_count)
{
  constexpr int G = 64, U = 8, E = 1;
  constexpr int kStages = 3 * (kGridLevels - 1);  // blocks (level 1, r = 1 .. 3), (level 2, r = 1 .. 3); then the whole target
  const int gl = threadIdx.x & 63;
  const int nwaves = gridDim.x * 4;
  // the list entry is loaded together with the count (its slot exists whatever the count is): one round trip
  int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  int q = list_in[min(w, list_cap - 1)];
  float4 qp = list_pts[min(w, list_cap - 1)];
  const int nwork = *count_in;
  for (; w < nwork; w += nwaves, q = list_in[min(w, list_cap - 1)], qp = list_pts[min(w, list_cap - 1)])
  {
    const float qx = qp.x, qy = qp.y, qz = qp.z;
    GroupSelect<KMAX, G, U> sel;
    sel.reset();
    bool done = false, far = false;
    GridView gv1, gv2;
    grid_view(gv1, desc + 1, gp.cell_start[1], gp.sorted[1], qx, qy, qz);
    grid_view(gv2, desc + 2, gp.cell_start[2], gp.sorted[2], qx, qy, qz);
    // every point closer than r cells (minus a 0.1 % guard for the float cell assignment) is in block (level, r)
    auto proven = [&](int stage) {
      const GridView& gv = stage < 3 ? gv1 : gv2;
      const float br = ((float)(1 + stage % 3) - 0.001f) * gv.g.cell;
      return gv.outd2 + br * br;
    };
    // Upper bound of the k-th distance (+inf: none yet), from the first stage and then from every scan that did
    // not settle the query: the first block whose proven radius exceeds it settles the query for certain, so the
    // search starts there -- one fetch of row bounds, one scan.  Without a bound the blocks are tried in order;
    // one that holds fewer than k points is not scanned.  The last "block" is the whole target.
    float ub = qp.w;
    int stage = 0;
    if (ub != INFINITY)
      while (stage < kStages - 1 && !(proven(stage) > ub)) ++stage;
#pragma unroll 1
    for (; stage <= kStages && !done; ++stage)
    {
      BlockRuns<G, E> runs;
      float bound2 = INFINITY;
      const float4* src = gp.sorted[0];
      if (stage < kStages)
      {
        const bool l1 = stage < 3;
        GridView gv;
        gv.g = l1 ? gv1.g : gv2.g;
        gv.cell_start = l1 ? gv1.cell_start : gv2.cell_start;
        gv.sorted = l1 ? gv1.sorted : gv2.sorted;
        gv.cx = l1 ? gv1.cx : gv2.cx; gv.cy = l1 ? gv1.cy : gv2.cy; gv.cz = l1 ? gv1.cz : gv2.cz;
        gv.outd2 = l1 ? gv1.outd2 : gv2.outd2;
        runs.build(gv, 1 + stage % 3, gl, true);
        bound2 = proven(stage);
        src = gv.sorted;
      }
      else
      {
        runs.whole((uint32_t)desc->npoints, gl);
        if (gl == 0) atomicAdd(exhaustive_count, 1);
      }
      const bool few = runs.total < (uint32_t)k;  // cannot hold k neighbours
      if (runs.covered || (!few && (ub == INFINITY || bound2 > ub || stage == kStages - 1)))
      {
        search_block<KMAX, G, U, E>(sel, runs, src, k, gl, qx, qy, qz);
        if (runs.covered || sel.count_below(bound2, k) >= k) done = true;
        else if (bound2 > far_d2) { far = true; done = true; }
        else
        {
#pragma unroll
          for (int s = 0; s < KMAX; ++s)
            if (s == k - 1) ub = key_d2(sel.best[s]);
        }
      }
      // fewer than k points inside a radius beyond the rejection distance
      else if (few && bound2 > far_d2) { far = true; done = true; }
    }
    if (gl == 0)
    {
      int cnt = 0;
#pragma unroll
      for (int s = 0; s < KMAX; ++s)
        if (s < k)
        {
          knn_idx[(size_t)s * cap + q] = key_idx(sel.best[s]);
          knn_d2[(size_t)s * cap + q] = key_d2(sel.best[s]);
          if (sel.best[s] != kKeyEmpty) ++cnt;
        }
      knn_cnt[q] = far ? kKnnFar : cnt;
    }
  }
}

// ------------------------------------------------------------------------------------------
template <int KMAX, int TYPE>
__global__ __launch_bounds__(kModelBlock) void k_model(const float4* __restrict__ queries, int nq, MatchConst c, const int* __restrict__ knn_idx,
                                                       const float* __restrict__ knn_d2, const int* __restrict__ knn_cnt,
                                                       const float4* __restrict__ xyzl, double* __restrict__ rec,
                                                       uint8_t* __restrict__ status, int cap, int* __restrict__ hist)
{
  __shared__ int lh[LSA_MATCH_NSTATUS];
  __shared__ float4 nb[(TYPE == LSA_EDGE ? KMAX : 1) * kModelBlock];  // edge candidates staged in LDS
  __shared__ float nd[(TYPE == LSA_EDGE ? KMAX : 1) * kModelBlock];
  if (threadIdx.x < LSA_MATCH_NSTATUS) lh[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq)
  {
    const int n = c.bad_param ? 0 : knn_cnt[i];
    const int st = fit_model<KMAX, TYPE>(
      queries[2 * (size_t)i], c, n, [&](int s) { return knn_idx[(size_t)s * cap + i]; }, [&](int s) { return knn_d2[(size_t)s * cap + i]; }, xyzl, nb, nd,
      kModelBlock, threadIdx.x, rec, cap, i);
    status[i] = (uint8_t)st;
    atomicAdd(&lh[st], 1);
  }
  __syncthreads();
  if (threadIdx.x < LSA_MATCH_NSTATUS && lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

template <int KMAX>
void launch_knn(lsa_ctx* ctx, const lsa_point_t* q, int nq, const Rigid& pose, int k, float far_d2, int type, int ti, hipStream_t st, int* hist)
{
  Target& t = ctx->target[ti];
  MatchBuf& mb = ctx->match[type];
  GridPtrs gp;
  for (int l = 0; l < kGridLevels; ++l) { gp.cell_start[l] = t.lv[l].cell_start; gp.sorted[l] = t.lv[l].sorted; }
  const float4* q4 = reinterpret_cast<const float4*>(q);
  int* cntA = hist + LSA_MATCH_NSTATUS;  // queries handed from the first to the second stage
  int* cntB = cntA + 1;                  // queries that needed the exhaustive scan (diagnostics)
  int* listA = mb.slow_list;
  const char* nf = type == LSA_EDGE ? "knn_fine_edge" : type == LSA_PLANE ? "knn_fine_plane" : "knn_fine_blob";
  const char* nc = type == LSA_EDGE ? "knn_coarse_edge" : type == LSA_PLANE ? "knn_coarse_plane" : "knn_coarse_blob";
  {
    // algorithmic bytes: query point in, k candidate points examined at least, k (index, distance) pairs out
    ProfScope ps(ctx, nf, (double)nq * (32 + k * 16 + k * 8), st);
    const int lanes = ctx->knn_lanes[type];
    const int rounds = ctx->knn_rounds[type];
#define LSA_FIRST(G, R)                                                                                                                     \
  hipLaunchKernelGGL((k_knn_first<KMAX, G, R>), dim3((int)(((size_t)nq * G + 255) / 256)), dim3(256), 0, st, q4, nq, pose, k, far_d2, t.desc, gp, \
                     mb.knn_idx, mb.knn_d2, mb.knn_cnt, mb.cap, cntA, listA, mb.slow_pts)
    if (lanes >= 32) { if (rounds >= 3) LSA_FIRST(32, 3); else LSA_FIRST(32, 2); }
    else if (lanes >= 16) { if (rounds >= 3) LSA_FIRST(16, 3); else LSA_FIRST(16, 2); }
    else { if (rounds >= 3) LSA_FIRST(8, 3); else LSA_FIRST(8, 2); }
#undef LSA_FIRST
  }
  {
    // the deferred share is only known on the device: no bytes are credited to this stage
    ProfScope ps(ctx, nc, 0., st);
    hipLaunchKernelGGL((k_knn_second<KMAX>), dim3(512), dim3(256), 0, st, (const int*)listA, (const float4*)mb.slow_pts, (const int*)cntA, mb.cap, k,
                       far_d2, t.desc, gp, mb.knn_idx, mb.knn_d2, mb.knn_cnt, mb.cap, cntB);
  }
}

template <int KMAX, int TYPE>
void launch_model(lsa_ctx* ctx, const lsa_point_t* q, int nq, const MatchConst& mc, int type, int ti, hipStream_t st, int* hist)
{
  Target& t = ctx->target[ti];
  MatchBuf& mb = ctx->match[type];
  hipLaunchKernelGGL((k_model<KMAX, TYPE>), dim3((nq + kModelBlock - 1) / kModelBlock), dim3(kModelBlock), 0, st,
                     reinterpret_cast<const float4*>(q), nq, mc, mb.knn_idx, mb.knn_d2, mb.knn_cnt, t.xyzl, mb.rec, mb.status, mb.cap, hist);
}

}  // namespace

namespace lsa
{

// The exact k nearest neighbours of nq queries in target ti, into the type's match buffer.  k <= 5 takes the <5>
// instantiation (planes: 5 neighbours, fewer registers, more waves in flight) -- and so does the overlap estimator's
// k = 1, whose speed depends on it.
void enqueue_staged_knn(lsa_ctx* ctx, const lsa_point_t* q, int nq, const Rigid& pose, int k, float far_d2, int type, int ti, hipStream_t st, int* hist)
{
  ctx->match[type].knn_n = nq;
  ctx->match[type].knn_k = k;
  if (k <= 5) launch_knn<5>(ctx, q, nq, pose, k, far_d2, type, ti, st, hist);
  else if (k <= 8) launch_knn<8>(ctx, q, nq, pose, k, far_d2, type, ti, st, hist);
  else launch_knn<16>(ctx, q, nq, pose, k, far_d2, type, ti, st, hist);
}

// Enqueues one prepared match as the staged kernels (first kNN stage -> second stage -> model fit) on `st`.
void enqueue_staged_match(lsa_ctx* ctx, const MatchPrep& mp, const double pose[16], hipStream_t st)
{
  const int type = mp.type, ti = mp.ti, nq = mp.nq;
  const MatchConst& mc = mp.mc;
  const lsa_point_t* q = mp.queries;
  int* hist = mp.hist;
  Rigid rp;
  row_major_to_rt(pose, rp.R, rp.t);
  if (!mc.bad_param) enqueue_staged_knn(ctx, q, nq, rp, mc.k, mp.far_d2, type, ti, st, hist);
  {
    ProfScope ps(ctx, type == LSA_EDGE ? "model_edge" : type == LSA_PLANE ? "model_plane" : "model_blob",
                 (double)nq * (32 + mc.k * 8 + mc.k * 16 + 136), st);
    if (type == LSA_EDGE)
    {
      if (mc.k <= 8) launch_model<8, LSA_EDGE>(ctx, q, nq, mc, type, ti, st, hist);
      else launch_model<16, LSA_EDGE>(ctx, q, nq, mc, type, ti, st, hist);
    }
    else if (type == LSA_PLANE)
    {
      if (mc.k <= 8) launch_model<8, LSA_PLANE>(ctx, q, nq, mc, type, ti, st, hist);
      else launch_model<16, LSA_PLANE>(ctx, q, nq, mc, type, ti, st, hist);
    }
    else
    {
      if (mc.k <= 8) launch_model<8, LSA_BLOB>(ctx, q, nq, mc, type, ti, st, hist);
      else launch_model<16, LSA_BLOB>(ctx, q, nq, mc, type, ti, st, hist);
    }
  }
}

}  // namespace lsa

extern "C" {

int lsa_set_knn_rounds(lsa_ctx* ctx, int type, int rounds)
{
  if (!ctx || type < 0 || type > 2 || rounds < 2 || rounds > 3) return LSA_E_ARG;
  ctx->knn_rounds[type] = rounds;
  return LSA_OK;
}

int lsa_set_knn_lanes(lsa_ctx* ctx, int type, int lanes)
{
  if (!ctx || type < 0 || type > 2 || lanes < 1) return LSA_E_ARG;
  ctx->knn_lanes[type] = lanes;
  return LSA_OK;
}

}  // extern "C"
