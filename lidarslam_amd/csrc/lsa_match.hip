// lsa_match.hip -- the C ABI of KeypointsMatcher::BuildMatchResiduals: lsa_match*, the histogram ring, download and
// upload of the residual records, diagnostics.  The search itself is lsa_match_fused.hip (one launch per ICP
// iteration, production) or lsa_match_staged.hip (cross-check); the targets and their grids are lsa_target.hip.
#include <cmath>
#include <cstring>
#include "lsa_ctx.h"
#include "lsa_device_math.h"
#include "lsa_knn.h"
#include "lsa_match_internal.h"

using namespace lsa;

namespace
{

__global__ void k_fill_status(uint8_t* __restrict__ status, double* __restrict__ rec, int cap, int n, uint8_t v)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { status[i] = v; rec[(size_t)15 * cap + i] = 0.; }
}

__global__ void k_records_to_aos(const double* __restrict__ rec, const uint8_t* __restrict__ status, int cap, int n, double* __restrict__ out,
                                 double* __restrict__ weights)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool ok = status[i] == LSA_MATCH_SUCCESS;
  if (out)
    for (int f = 0; f < 16; ++f) out[(size_t)i * 16 + f] = ok ? rec[(size_t)f * cap + i] : 0.;
  weights[i] = ok ? rec[(size_t)15 * cap + i] : 0.;
}

}  // namespace

// block `pos` of a type's histogram ring: 16 ints
static int* hist_block(lsa_ctx* ctx, int type, int pos) { return ctx->hist_dev + ((size_t)type * kHistRing + pos) * 16; }

// Next block of the type's histogram ring.  The ring is cleared one half at a time, when the position enters the
// half: everything that used those blocks finished long ago (the streams were joined and the host has read the
// results of those matches since), and the blocks of the last kHistRing / 2 matches stay readable
// (lsa_match_histogram).
int lsa::next_hist_block(lsa_ctx* ctx, int type, hipStream_t st, int** hist)
{
  constexpr int half = kHistRing / 2;
  ++ctx->hist_serial[type];
  if (++ctx->hist_pos[type] >= kHistRing) ctx->hist_pos[type] = 0;
  const int pos = ctx->hist_pos[type];
  if (pos % half == 0) LSA_HIP(ctx, hipMemsetAsync(hist_block(ctx, type, pos), 0, (size_t)half * 16 * sizeof(int), st));
  *hist = hist_block(ctx, type, pos);
  return LSA_OK;
}

// the diagnostics readers: waits for the context's stream, then copies n ints from `offset` ints into block `pos`
static hipError_t read_hist_block(lsa_ctx* ctx, int type, int pos, int offset, int* out, int n)
{
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  return e != hipSuccess ? e : hipMemcpy(out, hist_block(ctx, type, pos) + offset, (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
}

// a type's neighbour count as asked for, and whether its parameters are BAD_MODEL_PARAMETRIZATION for every keypoint
struct TypeParams { int k; bool bad; };
static TypeParams type_params(const lsa_match_params_t& p, int type)
{
  if (type == LSA_EDGE) return {p.edge_nb_neighbors, p.edge_nb_neighbors < 2 || p.edge_min_nb_neighbors < 2};
  if (type == LSA_PLANE) return {p.plane_nb_neighbors, p.plane_nb_neighbors < 3};
  return {p.blob_nb_neighbors, p.blob_nb_neighbors < 4};
}

extern "C" {

int lsa_set_fused_match(lsa_ctx* ctx, int on)
{
  if (!ctx) return LSA_E_ARG;
  ctx->fused_match = on != 0;
  ctx->fused_model = on != 2;
  return LSA_OK;
}

// Resolves the parameters of one keypoint type's match and takes its histogram block.  Returns 1 when there is
// something to search (keypoints and a non-empty target), 0 when the match is complete as it stands.
static int match_prepare(lsa_ctx* ctx, int slot, int type, int query_set, const lsa_match_params_t* p, hipStream_t st, MatchPrep& out)
{
  const int nq = ctx->kp_n[query_set][type];
  MatchBuf& mb = ctx->match[type];
  int* hist = nullptr;
  {
    const int rc = next_hist_block(ctx, type, st, &hist);
    if (rc) return rc;
  }
  mb.k = nq;
  mb.knn_n = 0;  // until a search that leaves its lists in memory is enqueued for it
  mb.sat = p->saturation_distance;
  mb.valid = true;
  ctx->last_match_type = type;
  if (nq == 0) return 0;
  const int ti = slot * 3 + type;
  Target& t = ctx->target[ti];
  if (t.m == 0)
  {
    // empty target: MatchingResults::Reset leaves every keypoint UNKOWN and the histogram empty
    // (KeypointsMatcher.cxx:53-58)
    hipLaunchKernelGGL(k_fill_status, dim3((nq + 255) / 256), dim3(256), 0, st, mb.status, mb.rec, mb.cap, nq, (uint8_t)LSA_MATCH_UNKOWN);
    return 0;
  }
  MatchConst mc;
  mc.type = type;
  mc.single_edge_per_ring = p->single_edge_per_ring;
  mc.min_neighbors = p->edge_min_nb_neighbors;
  mc.max_dist2 = p->max_neighbors_distance * p->max_neighbors_distance;
  mc.planarity = p->planarity_threshold;
  const TypeParams tp = type_params(*p, type);
  mc.k = tp.k;
  mc.bad_param = tp.bad ? 1 : 0;
  mc.max_model_err = type == LSA_EDGE ? p->edge_max_model_error : type == LSA_PLANE ? p->plane_max_model_error : 0.;
  const double e2 = p->edge_max_model_error * p->edge_max_model_error;
  mc.ransac_sq_inlier = (float)e2;
  if (mc.k < 1) mc.k = 1;
  // planes and blobs use all k neighbours and reject the match when the k-th is too far: the search may
  // stop as soon as that is certain (and the target is known to hold at least k points).  Edge matches
  // filter their neighbours first, so they need the true k nearest whatever the distance.
  float far_d2 = INFINITY;
  if (type != LSA_EDGE && t.m >= mc.k) far_d2 = (float)(mc.max_dist2 * 1.0001);
  out.type = type;
  out.ti = ti;
  out.queries = ctx->kp[query_set][type];
  out.nq = nq;
  out.mc = mc;
  out.far_d2 = far_d2;
  out.hist = hist;
  return 1;
}

static int match_check(lsa_ctx* ctx, int type, const lsa_match_params_t* p)
{
  if (type_params(*p, type).k > kKnnMax) return ctx->fail(LSA_E_ARG, "lsa_match: more than 16 neighbours requested");
  return LSA_OK;
}

int lsa_match(lsa_ctx* ctx, int slot, int type, int query_set, const lsa_match_params_t* p, const double pose[16], int histogram[LSA_MATCH_NSTATUS])
{
  if (!ctx || !p || !pose || slot < 0 || slot > 1 || type < 0 || type > 2 || query_set < 0 || query_set > 2)
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_match: bad argument") : LSA_E_ARG;
  int hist3[3 * LSA_MATCH_NSTATUS];
  const int rc = lsa_match_types(ctx, slot, 1u << type, query_set, p, pose, histogram ? hist3 : nullptr);
  if (rc == LSA_OK && histogram) std::memcpy(histogram, hist3 + type * LSA_MATCH_NSTATUS, LSA_MATCH_NSTATUS * sizeof(int));
  return rc;
}

static int match_types_impl(lsa_ctx* ctx, int slot, unsigned type_mask, int query_set, const lsa_match_params_t* p, const double pose[16], int* histograms,
                            const InterpConst* undistort, int link = -1, bool link_undistorts = false)
{
  if (!ctx || !p || (!pose && link < 0) || slot < 0 || slot > 1 || (type_mask & ~7u) || query_set < 0 || query_set > 2)
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_match_types: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  if (histograms) std::memset(histograms, 0, 3 * LSA_MATCH_NSTATUS * sizeof(int));
  int types[3], nt = 0;
  for (int k = 0; k < 3; ++k)
    if ((type_mask >> k) & 1u)
    {
      int rc = match_check(ctx, k, p);
      if (rc) return rc;
      rc = ensure_match(ctx, k, ctx->kp_n[query_set][k]);  // may reallocate (and synchronise) before anything is forked
      if (rc) return rc;
      types[nt++] = k;
    }
  if (nt == 0) return LSA_OK;
  {
    const int rc = flush_grids(ctx);
    if (rc) return rc;
  }
  if (ctx->fused_match)
  {
    // one launch for all the types (+ the tail launch), on the context's stream
    MatchPrep preps[3];
    int np = 0;
    for (int i = 0; i < nt; ++i)
    {
      if (link >= 0)
      {
        // should the iteration be called off, what it announces here is taken back (lsa_icp_cancel)
        lsa_ctx::LinkSaved& sv = ctx->link_saved[link];
        const int k = types[i];
        sv.mask |= 1u << k;
        sv.sat[k] = ctx->match[k].sat; sv.k[k] = ctx->match[k].k; sv.valid[k] = ctx->match[k].valid;
        sv.hist_pos[k] = ctx->hist_pos[k]; sv.hist_serial[k] = ctx->hist_serial[k];
      }
      const int rc = match_prepare(ctx, slot, types[i], query_set, p, ctx->stream, preps[np]);
      if (rc < 0) return rc;
      if (rc > 0) ++np;
    }
    if (np > 0)
    {
      const int rc = enqueue_fused_match(ctx, preps, np, pose, ctx->stream, undistort, link, link_undistorts);
      if (rc) return rc;
    }
  }
  else
  {
    // fork: the first type stays on the context stream, the others run beside it.  A single type's kernels
    // leave most of the 256 CUs idle (a few thousand queries, latency bound), so the types overlap almost fully.
    for (int i = 0; i + 1 < nt; ++i)
      if (!ctx->side_stream[i]) LSA_HIP(ctx, hipStreamCreateWithFlags(&ctx->side_stream[i], hipStreamNonBlocking));  // lsa_ctx_create: why not there
    if (nt > 1) LSA_HIP(ctx, hipEventRecord(ctx->ev_fork, ctx->stream));
    for (int i = 0; i < nt; ++i)
    {
      hipStream_t st = i == 0 ? ctx->stream : ctx->side_stream[i - 1];
      if (i > 0) LSA_HIP(ctx, hipStreamWaitEvent(st, ctx->ev_fork, 0));
      MatchPrep mp;
      const int rc = match_prepare(ctx, slot, types[i], query_set, p, st, mp);
      if (rc < 0) return rc;
      if (rc > 0) enqueue_staged_match(ctx, mp, pose, st);
      if (i > 0) LSA_HIP(ctx, hipEventRecord(ctx->ev_join[i - 1], st));
    }
    for (int i = 1; i < nt; ++i) LSA_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_join[i - 1], 0));
  }
  if (histograms)
  {
    int* hp = reinterpret_cast<int*>(ctx->host_pinned) + 32;
    for (int i = 0; i < nt; ++i)
      LSA_HIP(ctx, hipMemcpyAsync(hp + types[i] * 16, hist_block(ctx, types[i], ctx->hist_pos[types[i]]), 16 * sizeof(int),
                                  hipMemcpyDeviceToHost, ctx->stream));
    LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < nt; ++i)
      for (int s = 0; s < LSA_MATCH_NSTATUS; ++s) histograms[types[i] * LSA_MATCH_NSTATUS + s] = hp[types[i] * 16 + s];
  }
  return LSA_OK;
}

int lsa_match_types(lsa_ctx* ctx, int slot, unsigned type_mask, int query_set, const lsa_match_params_t* p, const double pose[16], int* histograms)
{
  return match_types_impl(ctx, slot, type_mask, query_set, p, pose, histograms, nullptr);
}

// Whether the search kernel reaches every keypoint of the working set, so that an undistortion can be done inside it: the
// one-launch form, every type that has keypoints asked for, with a target and with valid parameters (a type that is not
// searched would keep its distortion)
static bool search_reaches_every_keypoint(lsa_ctx* ctx, int slot, unsigned type_mask, const lsa_match_params_t* p)
{
  bool reach = ctx->fused_match;
  for (int k = 0; k < 3 && reach; ++k)
  {
    if (ctx->kp_n[LSA_SET_WORKING][k] <= 0) continue;
    const TypeParams tp = type_params(*p, k);
    reach = ((type_mask >> k) & 1u) && ctx->target[slot * 3 + k].m > 0 && !tp.bad && tp.k <= kKnnMax;
  }
  return reach;
}

int lsa_match_types_undistorted(lsa_ctx* ctx, int slot, unsigned type_mask, const lsa_match_params_t* p, const double pose[16], int* histograms, const double H0[16],
                                const double H1[16], double t0, double t1)
{
  if (!ctx || !p || !pose || !H0 || !H1 || slot < 0 || slot > 1 || (type_mask & ~7u))
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_match_types_undistorted: bad argument") : LSA_E_ARG;
  if (!search_reaches_every_keypoint(ctx, slot, type_mask, p))
  {
    const int rc = lsa_undistort(ctx, H0, H1, t0, t1);
    return rc ? rc : match_types_impl(ctx, slot, type_mask, LSA_SET_WORKING, p, pose, histograms, nullptr);
  }
  const InterpConst ic = make_interp_const(H0, H1, t0, t1);
  return match_types_impl(ctx, slot, type_mask, LSA_SET_WORKING, p, pose, histograms, &ic);
}

int lsa_match_types_linked(lsa_ctx* ctx, int slot, unsigned type_mask, int query_set, const lsa_match_params_t* p, int undistort)
{
  if (!ctx || !p || slot < 0 || slot > 1 || (type_mask & ~7u) || query_set < 0 || query_set > 2)
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_match_types_linked: bad argument") : LSA_E_ARG;
  if (ctx->link_current < 0) return ctx->fail(LSA_E_STATE, "lsa_match_types_linked: no link to wait behind (lsa_icp_link)");
  // only the one-launch form reads a link; an undistortion must reach every keypoint of the working set (otherwise it is a
  // launch of its own, which the caller has to enqueue once the motion is known)
  if (!ctx->fused_match || !ctx->fused_model) return 1;
  if (undistort && (query_set != LSA_SET_WORKING || !search_reaches_every_keypoint(ctx, slot, type_mask, p))) return 1;
  for (int k = 0; k < 3; ++k)
    if (((type_mask >> k) & 1u) && ctx->kp_n[query_set][k] > 0 && ctx->target[slot * 3 + k].m <= 0) return 1;  // (an empty target is answered by a fill, not by the search)
  return match_types_impl(ctx, slot, type_mask, query_set, p, nullptr, nullptr, nullptr, ctx->link_current, undistort != 0);
}

int lsa_download_match(lsa_ctx* ctx, int type, uint8_t* status, double* weights, double* records, int capacity)
{
  if (!ctx || type < 0 || type > 2 || !status || !weights) return ctx ? ctx->fail(LSA_E_ARG, "lsa_download_match: bad argument") : LSA_E_ARG;
  MatchBuf& mb = ctx->match[type];
  if (!mb.valid) return 0;
  const int n = std::min(capacity, mb.k);
  if (n <= 0) return 0;
  const size_t bytes = (size_t)n * (16 + 1) * sizeof(double);
  int rc = ensure_scratch(ctx, bytes);
  if (rc) return rc;
  double* drec = (double*)ctx->scratch_out;
  double* dw = drec + (size_t)n * 16;
  hipLaunchKernelGGL(k_records_to_aos, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, mb.rec, mb.status, mb.cap, n, records ? drec : nullptr, dw);
  if (records) LSA_HIP(ctx, hipMemcpyAsync(records, drec, (size_t)n * 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(weights, dw, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipMemcpyAsync(status, mb.status, (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return n;
}

int lsa_upload_match(lsa_ctx* ctx, int type, const uint8_t* status, const double* records, int n, double saturation)
{
  if (!ctx || type < 0 || type > 2 || n < 0 || (n > 0 && (!status || !records)) || !std::isfinite(saturation))
    return ctx ? ctx->fail(LSA_E_ARG, "lsa_upload_match: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  MatchBuf& mb = ctx->match[type];
  int rc = ensure_match(ctx, type, n);  // (outgrown buffers are retired: launches in flight keep them)
  if (rc) return rc;
  if (n > 0)
  {
    // rows as lsa_download_match hands them out -> the SoA layout of the match buffer, rejected rows as given
    std::vector<double> soa((size_t)16 * n);
    for (int i = 0; i < n; ++i)
      for (int f = 0; f < 16; ++f) soa[(size_t)f * n + i] = records[(size_t)i * 16 + f];
    LSA_HIP(ctx, hipMemcpy2DAsync(mb.rec, (size_t)mb.cap * sizeof(double), soa.data(), (size_t)n * sizeof(double), (size_t)n * sizeof(double), 16,
                                  hipMemcpyHostToDevice, ctx->stream));
    LSA_HIP(ctx, hipMemcpyAsync(mb.status, status, (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  mb.k = n;
  mb.sat = saturation;
  mb.valid = true;
  return LSA_OK;
}

// Test hook.  The lists live on the device as [kKnnMax][cap] (slot s of query q at s * cap + q): copied as they are,
// one strided copy each, and turned into rows per query on the host.
int lsa_download_knn(lsa_ctx* ctx, int type, int* idx, float* d2, int* cnt, int capacity)
{
  static_assert(LSA_KNN_MAX == kKnnMax, "the header's row length is the buffers'");
  if (!ctx || type < 0 || type > 2 || !idx || !d2 || !cnt) return ctx ? ctx->fail(LSA_E_ARG, "lsa_download_knn: bad argument") : LSA_E_ARG;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  const MatchBuf& mb = ctx->match[type];
  const int n = std::min(capacity, mb.knn_n);
  if (n <= 0) return 0;
  std::vector<int> si((size_t)kKnnMax * n);
  std::vector<float> sd((size_t)kKnnMax * n);
  LSA_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the staged form's side streams have been joined into it)
  LSA_HIP(ctx, hipMemcpy2D(si.data(), (size_t)n * sizeof(int), mb.knn_idx, (size_t)mb.cap * sizeof(int), (size_t)n * sizeof(int), kKnnMax, hipMemcpyDeviceToHost));
  LSA_HIP(ctx, hipMemcpy2D(sd.data(), (size_t)n * sizeof(float), mb.knn_d2, (size_t)mb.cap * sizeof(float), (size_t)n * sizeof(float), kKnnMax, hipMemcpyDeviceToHost));
  LSA_HIP(ctx, hipMemcpy(cnt, mb.knn_cnt, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  const int k = std::min(std::max(mb.knn_k, 0), kKnnMax);
  for (int q = 0; q < n; ++q)
    for (int s = 0; s < kKnnMax; ++s)
    {
      // slots the search was not asked for hold whatever an earlier one left: handed out as "none"
      idx[(size_t)q * kKnnMax + s] = s < k ? si[(size_t)s * n + q] : -1;
      d2[(size_t)q * kKnnMax + s] = s < k ? sd[(size_t)s * n + q] : INFINITY;
    }
  return n;
}

long long lsa_match_serial(const lsa_ctx* ctx, int type)
{
  if (!ctx || type < 0 || type > 2) return LSA_E_ARG;
  return ctx->hist_serial[type];
}

int lsa_match_histogram(lsa_ctx* ctx, int type, long long serial, int histogram[LSA_MATCH_NSTATUS])
{
  if (!ctx || type < 0 || type > 2 || !histogram) return ctx ? ctx->fail(LSA_E_ARG, "lsa_match_histogram: bad argument") : LSA_E_ARG;
  const long long back = ctx->hist_serial[type] - serial;
  if (serial <= 0 || back < 0 || back >= kHistRing / 2) return ctx->fail(LSA_E_STATE, "lsa_match_histogram: that match is not (or no longer) in the ring");
  const int pos = (int)(((long long)ctx->hist_pos[type] - back) % kHistRing + kHistRing) % kHistRing;
  LSA_HIP(ctx, hipSetDevice(ctx->device));
  LSA_HIP(ctx, read_hist_block(ctx, type, pos, 0, histogram, LSA_MATCH_NSTATUS));
  return LSA_OK;
}

int lsa_match_slow_queries(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  int v = 0;
  const int type = ctx->last_match_type;
  return read_hist_block(ctx, type, ctx->hist_pos[type], LSA_MATCH_NSTATUS, &v, 1) == hipSuccess ? v : LSA_E_HIP;
}

int lsa_match_route_stats(lsa_ctx* ctx, int type, int out[8])
{
  if (!ctx || type < 0 || type > 2 || !out) return LSA_E_ARG;
  return read_hist_block(ctx, type, ctx->hist_pos[type], LSA_MATCH_NSTATUS, out, 8) == hipSuccess ? LSA_OK : LSA_E_HIP;
}

int lsa_match_trace(lsa_ctx* ctx, unsigned long long* out, int blocks)
{
  if (!ctx || !out || blocks < 0 || blocks > 8192 || !ctx->trace_dev) return LSA_E_ARG;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess) return LSA_E_HIP;
  if (hipMemcpy(out, ctx->trace_dev, (size_t)blocks * 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return LSA_E_HIP;
  return LSA_OK;
}

int lsa_match_exhaustive_queries(lsa_ctx* ctx)
{
  if (!ctx) return LSA_E_ARG;
  int v = 0;
  const int type = ctx->last_match_type;
  return read_hist_block(ctx, type, ctx->hist_pos[type], LSA_MATCH_NSTATUS + 1, &v, 1) == hipSuccess ? v : LSA_E_HIP;
}

}  // extern "C"
