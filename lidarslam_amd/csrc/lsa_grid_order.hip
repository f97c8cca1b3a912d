// lsa_grid_order.hip -- the device map in the reference's container order ("Ordered" = 0, see the head of
// lsa_device_grid.hip): the record every modification leaves, its replay on the host's keys-only copy of the containers
// (host/lsa_map_order.h), and the upload of that copy's iteration order as places in the sorted array.
#include <vector>
#include "lsa_grid.h"

using namespace lsa;

namespace
{
// ---- the reference's container order ("Ordered" = 0) -------------------------------------------------------------------
// The host uploads the keys in the iteration order of its copy of the containers; every one becomes its place in the
// sorted array.  The extractions then compact over r = 0 .. n-1 and read voxel perm[r]: the same predicates, the same
// emitters, another order.
__global__ __launch_bounds__(256) void k_order_perm(const u64* __restrict__ okeys, int n, const u64* __restrict__ keys, const int* __restrict__ st,
                                                    int* __restrict__ perm)
{
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int N = st[kStN];
  const int at = lower_bound_u64(keys, N, okeys[r]);
  perm[r] = at < N ? at : (N > 0 ? N - 1 : 0);  // (never taken: the host's key set is the map's)
}
}  // namespace

namespace lsa
{
// the last modification's record replayed on the shadow (waits for that modification)
int apply_record(lsa_device_grid* g)
{
  if (!g->rec_kind) return LSA_OK;
  G_HIP(hipEventSynchronize(g->ev_rec));
  const int kind = g->rec_kind;
  g->rec_kind = 0;
  g->order_stale = true;
  const int* s = g->rec_st;
  g->rec_voxels = s[kStN];
  if (kind == kRecAdd || kind == kRecRoll)
  {
    // Add rolls first (RollingGrid.cxx:166-172): the move it made, then the keys it created
    const int off[3] = {s[kStOff], s[kStOff + 1], s[kStOff + 2]};
    g->shadow.Roll(off, g->rec_grid);
  }
  if (kind == kRecAdd)
  {
    const int created = s[kStNew];
    if (created < 0 || 2 * (size_t)created > g->rec_cap) return g->ctx->fail(LSA_E_STATE, "lsa_device_grid: bad record of an insertion");
    // {key, first arrival}: operator[] inserts a key at its first point (:206-212), so the order of insertion is that of arrival
    std::vector<std::pair<unsigned, u64>> fresh((size_t)created);
    for (int i = 0; i < created; ++i) fresh[i] = {(unsigned)g->rec_host[2 * (size_t)i + 1], g->rec_host[2 * (size_t)i]};
    std::sort(fresh.begin(), fresh.end());
    for (const auto& f : fresh) g->shadow.Insert(f.second);
  }
  else if (kind == kRecDecay)
  {
    const int erased = s[kStRec];
    if (erased < 0 || (size_t)erased > g->rec_cap) return g->ctx->fail(LSA_E_STATE, "lsa_device_grid: bad record of a decay");
    // the keys themselves, now that their number is known (nothing has written the record's buffer since: every
    // modification replays the record before it is enqueued)
    if (erased > 0)
    {
      G_HIP(hipMemcpyAsync(g->rec_host, g->rec_dev, (size_t)erased * sizeof(u64), hipMemcpyDeviceToHost, g->stream));
      G_HIP(hipEventRecord(g->ev_rec, g->stream));
      G_HIP(hipEventSynchronize(g->ev_rec));
    }
    std::vector<u64> keys(g->rec_host, g->rec_host + erased);
    std::sort(keys.begin(), keys.end());
    g->shadow.Erase(keys);
  }
  return LSA_OK;
}

// RollingGrid::Clear (:51-56) on the shadow: the keys go, the bucket arrays stay.  A record still on its way is replayed
// first: the tables' bucket counts after the clear -- and with them the order of every later insertion -- are what the
// modifications before it made of them.
int forget_records(lsa_device_grid* g)
{
  const int rc = apply_record(g);
  if (rc) return rc;
  g->shadow.Clear();
  g->rec_voxels = 0;
  g->order_stale = true;
  return LSA_OK;
}

// room for a record of `entries` keys (the last record has been replayed)
int ensure_rec(lsa_device_grid* g, size_t entries)
{
  if (entries <= g->rec_cap) return LSA_OK;
  G_HIP(hipEventSynchronize(g->ev_rec));
  const size_t cap = std::max(2 * entries, (size_t)1 << 16);
  if (g->rec_host) G_HIP(hipHostFree(g->rec_host));
  g->rec_host = nullptr;
  retire_dev(g->ctx, g->rec_dev);
  g->rec_dev = nullptr;
  g->rec_cap = 0;
  G_HIP(hipHostMalloc((void**)&g->rec_host, cap * sizeof(u64), hipHostMallocDefault));
  G_HIP(hipMalloc((void**)&g->rec_dev, cap * sizeof(u64)));
  g->rec_cap = cap;
  return LSA_OK;
}

// the record of the modification just enqueued goes to the host behind it: the state, then `entries` keys
int send_record(lsa_device_grid* g, int kind, size_t entries)
{
  G_HIP(hipMemcpyAsync(g->rec_st, g->st, kStInts * sizeof(int), hipMemcpyDeviceToHost, g->stream));
  if (entries > 0) G_HIP(hipMemcpyAsync(g->rec_host, g->rec_dev, entries * sizeof(u64), hipMemcpyDeviceToHost, g->stream));
  G_HIP(hipEventRecord(g->ev_rec, g->stream));
  g->rec_kind = kind;
  g->rec_grid = g->GridSize;
  return LSA_OK;
}

// The order of the map as it is now, on the device, before an extraction: the records replayed, the keys in the shadow's
// iteration order uploaded and turned into places (on the grid's stream; ev_out follows, for extractions on the context's).
int ensure_order(lsa_device_grid* g)
{
  int rc = apply_record(g);
  if (rc) return rc;
  if (!g->order_stale) return LSA_OK;
  const int n = (int)g->shadow.Size();
  if (n != g->rec_voxels) return g->ctx->fail(LSA_E_STATE, "lsa_device_grid: the host's copy of the containers holds " + std::to_string(n) + " keys, the map " + std::to_string(g->rec_voxels) + " voxels");
  G_HIP(hipEventSynchronize(g->ev_order));  // the last upload out of order_host is over
  if (n > g->order_cap)
  {
    const int cap = std::max(2 * n, 1 << 16);
    if (g->order_host) G_HIP(hipHostFree(g->order_host));
    g->order_host = nullptr;
    retire_dev(g->ctx, g->order_dev);
    retire_dev(g->ctx, g->perm);
    g->order_dev = nullptr;
    g->perm = nullptr;
    g->order_cap = 0;
    G_HIP(hipHostMalloc((void**)&g->order_host, (size_t)cap * sizeof(u64), hipHostMallocDefault));
    G_HIP(hipMalloc((void**)&g->order_dev, (size_t)cap * sizeof(u64)));
    G_HIP(hipMalloc((void**)&g->perm, (size_t)cap * sizeof(int)));
    g->order_cap = cap;
  }
  g->shadow.Keys(g->order_host);
  G_HIP(hipStreamWaitEvent(g->stream, g->ev_sub, 0));  // an extraction on the context's stream may still read the places
  if (n > 0)
  {
    rc = ensure_map(g, std::max(g->n_upper, n));
    if (rc) return rc;
    G_HIP(hipMemcpyAsync(g->order_dev, g->order_host, (size_t)n * sizeof(u64), hipMemcpyHostToDevice, g->stream));
    hipLaunchKernelGGL(k_order_perm, dim3((n + 255) / 256), dim3(256), 0, g->stream, g->order_dev, n, g->buf[g->cur].keys, g->st, g->perm);
  }
  G_HIP(hipEventRecord(g->ev_order, g->stream));
  G_HIP(hipEventRecord(g->ev_out, g->stream));
  g->order_stale = false;
  g->order_n = n;
  return LSA_OK;
}
}  // namespace lsa
