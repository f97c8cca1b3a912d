// lsa_grid_add.hip -- the device map's Add (RollingGrid.cxx:160-318): the kernels of the seven launches, their launcher
// for up to three maps at a time, the batch scratch, and the staging and add entry points of the C ABI.  The data structure
// is described at the head of lsa_device_grid.hip.
#include <cfloat>
#include <cmath>
#include "lsa_grid.h"
#include "lsa_device_grid_io.h"
#include "lsa_device_math.h"

using namespace lsa;

namespace
{
constexpr u64 kNoKey = ~0ull;  // points outside the grid: sorted behind every voxel

// bounding box of the batch: ordered-int atomics into st[kStTmp .. +5]
__device__ __forceinline__ void d_batch_bbox(int bx, const float4* __restrict__ batch, int n, int* __restrict__ st)
{
  __shared__ float s_box[4][6];
  const int i = bx * blockDim.x + threadIdx.x;
  BoxF box;
  if (i < n)
  {
    const float4 a = batch[2 * (size_t)i];
    box = box_of_point(a.x, a.y, a.z);
  }
  box_block_send<4>(box, st + kStTmp, s_box);
}

// ---- Add (RollingGrid.cxx:160-318) in seven launches --------------------------------------------------------------------
// (The first version -- bounding box, roll decision, roll compaction, keys, library radix sort, heads, fold, compaction of
// the new voxels, merge, state -- was twenty-five dependent launches, and the next localization waits for the last of
// them.)  Seven: box -> keys of the batch + survivors of the roll counted -> runs of 4096 sorted in LDS -> runs merged by
// rank -> fold per voxel (straight off the sorted batch) -> map = surviving old voxels (re-keyed) merged with the new ones
// by rank -> state.  Nothing is decided in a launch of its own: every kernel works the roll's shift out for itself from the
// committed grid position and the batch's box, and the last kernel commits position and counts.
struct Shift
{
  int off[3];     // outer voxels the grid moves by (Roll, RollingGrid.cxx:117-157)
  float pos[3];   // grid position after the move
  bool any;
};
__device__ __forceinline__ Shift roll_shift(const GridParams& p, const int* __restrict__ st, int use_box)
{
  Shift s;
  const double halfGridSize = static_cast<double>(p.grid_size) / 2 * p.resolution_d;
  const float h = (float)halfGridSize;
  s.any = false;
#pragma unroll
  for (int d = 0; d < 3; ++d)
  {
    const float pos = __int_as_float(st[kStPosX + d]);
    int off = 0;
    if (use_box)
    {
      const float mnv = os2f(st[kStTmp + d]), mxv = os2f(st[kStTmp + 3 + d]);
      const float down = mnv - (pos - h);
      const float up = mxv - (pos + h);
      float o = (up + down) / 2.f;
      const float lo = fminf(down, 0.f), hi = fmaxf(up, 0.f);
      o = fminf(fmaxf(o, lo), hi);
      off = round_to_int(o / p.resolution);
    }
    s.off[d] = off;
    s.pos[d] = pos + (float)off * p.resolution;
    s.any = s.any || off != 0;
  }
  return s;
}
// A voxel's place in the order of the map, comparable between the grid before and after a move: (z, y, x) of the outer
// voxel in the coordinates BEFORE the move (biased, 21 bits each: a voxel that is about to enter the grid has coordinates
// outside of it), then the leaf index.  Without a move the outer index itself does.
struct VKey
{
  u64 hi;
  unsigned lo;
};
__device__ __forceinline__ bool vless(const VKey& a, const VKey& b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ u64 biased3(int x, int y, int z)
{
  auto c = [](int v) { const int lim = (1 << 20) - 1; return (u64)(unsigned)((v < -lim ? -lim : (v > lim ? lim : v)) + (1 << 20)); };
  return (c(z) << 42) | (c(y) << 21) | c(x);
}
__device__ __forceinline__ VKey vkey_of_old(u64 key, bool any, int g)
{
  VKey k;
  k.lo = (unsigned)(key & 0xffffffffull);
  int id = (int)(unsigned)(key >> 32);
  if (!any) { k.hi = (u64)(unsigned)id; return k; }
  const int z = id / (g * g); id -= z * g * g;
  const int y = id / g; const int x = id - y * g;
  k.hi = biased3(x, y, z);
  return k;
}
// the key of a voxel of the grid AFTER the move, in that order
__device__ __forceinline__ VKey vkey_of_new(u64 key, const Shift& s, int g)
{
  VKey k;
  k.lo = (unsigned)(key & 0xffffffffull);
  int id = (int)(unsigned)(key >> 32);
  if (!s.any) { k.hi = (u64)(unsigned)id; return k; }
  const int z = id / (g * g); id -= z * g * g;
  const int y = id / g; const int x = id - y * g;
  k.hi = biased3(x + s.off[0], y + s.off[1], z + s.off[2]);
  return k;
}
__device__ __forceinline__ int lower_bound_old(const u64* __restrict__ keys, int n, const VKey& t, bool any, int g)
{
  int lo = 0, hi = n;
  while (lo < hi)
  {
    const int mid = (lo + hi) >> 1;
    if (vless(vkey_of_old(keys[mid], any, g), t)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// The same within [lo, hi) -- the answer is known to lie in [lo, hi].
__device__ __forceinline__ int lower_bound_old_in(const u64* __restrict__ keys, int lo, int hi, const VKey& t, bool any, int g)
{
  while (lo < hi)
  {
    const int mid = (lo + hi) >> 1;
    if (vless(vkey_of_old(keys[mid], any, g), t)) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// ... and by a whole wavefront for ONE key (the same in every lane): 64 probes per round trip instead of one, three or four
// dependent loads for a map of a million voxels instead of twenty.  Every lane returns the answer.
__device__ __forceinline__ int lower_bound_old_wave(const u64* __restrict__ keys, int n, const VKey& t, bool any, int g)
{
  const int lane = threadIdx.x & 63;
  int lo = 0, hi = n;  // the answer lies in [lo, hi]
  while (hi - lo > 64)
  {
    const int step = (hi - lo + 64) / 65;  // >= 1; probes at lo + step * (lane + 1) - 1, clamped: non-decreasing along the lanes
    const int pos = min(hi - 1, lo + step * (lane + 1) - 1);
    const bool less = vless(vkey_of_old(keys[pos], any, g), t);
    const int c = __popcll(__ballot(less));  // the keys ascend: the probes below the target are the first c lanes'
    // the answer is beyond probe c - 1 and not beyond probe c
    const int nlo = c == 0 ? lo : min(hi - 1, lo + step * c - 1) + 1;
    const int nhi = c == 64 ? hi : min(hi - 1, lo + step * (c + 1) - 1);
    lo = nlo; hi = nhi;
  }
  const int pos = lo + lane;
  const bool less = pos < hi && vless(vkey_of_old(keys[pos], any, g), t);
  return lo + __popcll(__ballot(less));
}
// does the voxel survive the move, and under which key
__device__ __forceinline__ bool shifted_key(u64 k, const Shift& s, int g, u64& out)
{
  int id = (int)(unsigned)(k >> 32);
  int z = id / (g * g);
  id -= z * g * g;
  int y = id / g;
  int x = id - y * g;
  x -= s.off[0]; y -= s.off[1]; z -= s.off[2];
  if (x < 0 || y < 0 || z < 0 || x >= g || y >= g || z >= g) return false;
  out = ((u64)(unsigned)(z * g * g + y * g + x) << 32) | (k & 0xffffffffull);
  return true;
}

// launch 2: blocks [0, kblocks): the keys of the batch in the grid after the move; the others: 1024 old voxels each, which
// of them survive the move -- every voxel's rank among the survivors of its chunk, and the chunk's count
__device__ __forceinline__ void d_add_keys(int bx, const float4* __restrict__ batch, int n, int kblocks, GridParams p, const int* __restrict__ st, int use_box,
                                                  u64* __restrict__ keys, const u64* __restrict__ old_keys, int* __restrict__ old_local,
                                                  int* __restrict__ old_chunks, int ochunks)
{
  const Shift s = roll_shift(p, st, use_box);
  const int g = p.grid_size;
  if ((int)bx < kblocks)
  {
    const int i = bx * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = batch[2 * (size_t)i];
    const float pt[3] = {a.x, a.y, a.z};
    int out[3], in[3];
    bool inside = true;
#pragma unroll
    for (int d = 0; d < 3; ++d)
    {
      // voxelGridOrigin = VoxelGridPosition - int(GridSize / 2) * VoxelResolution (:177)
      const float origin = s.pos[d] - (float)((double)(g / 2) * p.resolution_d);
      out[d] = round_to_int((pt[d] - origin) / p.resolution);
      inside = inside && out[d] >= 0 && out[d] < g;
      const float center = (float)out[d] * p.resolution + origin;
      in[d] = round_to_int((pt[d] - center) / p.leaf);
    }
    const unsigned idx_out = (unsigned)(out[2] * g * g + out[1] * g + out[0]);
    const unsigned idx_in = (unsigned)(in[2] * g * g + in[1] * g + in[0]);  // possibly "negative": the reference's own index (:200-202)
    keys[i] = inside ? (((u64)idx_out << 32) | idx_in) : kNoKey;
    return;
  }
  __shared__ int wave_cnt[4];
  const int chunk = bx - kblocks;
  if (chunk >= ochunks) return;  // (a launch shared with a bigger map)
  const int N = st[kStN];
  int run = 0;
  for (int q = 0; q < 4; ++q)
  {
    const int i = chunk * 1024 + q * 256 + threadIdx.x;
    u64 nk;
    const bool keep = i < N && shifted_key(old_keys[i], s, g, nk);
    const u64 ballot = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) wave_cnt[wv] = __popcll(ballot);
    __syncthreads();
    int base = run;
    for (int w = 0; w < wv; ++w) base += wave_cnt[w];
    if (i < N) old_local[i] = base + __popcll(ballot & ((1ull << lane) - 1ull));
    run += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  }
  if (threadIdx.x == 0) old_chunks[chunk] = run;
}

// launch 3: runs of 4096 (key, arrival index) pairs sorted by one workgroup (bitonic; the pairs are unique, so the order
// is the stable order by key).  A thread holds four consecutive pairs in registers: of the 78 steps of the network, the
// 23 whose partner is one of the thread's own pairs are done in place, the 45 whose partner sits in another lane of the
// wavefront go through lane exchanges, and only the 10 that cross wavefronts go through LDS (two buffers, one barrier
// each).  (The first version did all 78 through LDS with a barrier each: 55 us a run.)
constexpr int kRun = 4096;
struct SortPair
{
  u64 k;
  unsigned i;
};
__device__ __forceinline__ bool pair_gt(const SortPair& a, const SortPair& b) { return a.k > b.k || (a.k == b.k && a.i > b.i); }
// the value of lane (lane ^ M) for one 32-bit word: DPP operands and gfx950's permlane swaps, no LDS crossbar
template <int M>
__device__ __forceinline__ unsigned word_xor(unsigned x, int lane)
{
  if (M == 1) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
  if (M == 2) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
  if (M == 4)
  {
    const unsigned up = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x104, 0xF, 0xF, true);  // row_shl:4: lane i <- i + 4
    const unsigned dn = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);  // row_shr:4: lane i <- i - 4
    return (lane & 4) ? dn : up;
  }
  if (M == 8) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xF, 0xF, true);   // row_ror:8
  if (M == 16)
  {
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);  // [0]: rows 0 0 2 2, [1]: rows 1 1 3 3
    return (lane & 16) ? r[0] : r[1];
  }
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);    // [0]: lower half twice, [1]: upper half twice
  return (lane & 32) ? r[0] : r[1];
}
template <int M>
__device__ __forceinline__ SortPair lane_xor(const SortPair& v, int lane)
{
  SortPair o;
  const unsigned lo = word_xor<M>((unsigned)(v.k & 0xffffffffull), lane), hi = word_xor<M>((unsigned)(v.k >> 32), lane);
  o.k = ((u64)hi << 32) | lo;
  o.i = word_xor<M>(v.i, lane);
  return o;
}
__device__ __forceinline__ void d_sort_runs(int bx, const u64* keys, int n, u64* out_keys, unsigned* __restrict__ out_idx)  // keys == out_keys: in place, run by run
{
  __shared__ u64 sk[2][kRun];
  __shared__ unsigned si[2][kRun];
  const int base = bx * kRun, t = threadIdx.x;
  if (base >= n) return;  // (a launch shared with a bigger batch)
  SortPair v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
  {
    const int i = base + 4 * t + e;
    v[e].k = i < n ? keys[i] : kNoKey;
    v[e].i = i < n ? (unsigned)i : 0xffffffffu;
  }
  int buf = 0;
  for (int k = 2; k <= kRun; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1)
    {
      if (j <= 2)
      {
        // partner = another pair of this thread (constant register indices: j = 1 pairs 0-1 and 2-3, j = 2 pairs 0-2 and 1-3)
        auto cx = [&](SortPair& a, SortPair& b, int pos) {
          const bool up = ((pos & k) == 0);
          if (pair_gt(a, b) == up) { const SortPair x = a; a = b; b = x; }
        };
        if (j == 1) { cx(v[0], v[1], 4 * t); cx(v[2], v[3], 4 * t + 2); }
        else { cx(v[0], v[2], 4 * t); cx(v[1], v[3], 4 * t + 1); }
      }
      else
      {
        const int tj = j >> 2;                  // the partner thread is t ^ tj, same place inside the thread
        const bool lower = (t & tj) == 0;
        SortPair o[4];
        if (tj < 64)
        {
          const int lane = t & 63;
          // one of six code paths, chosen by a scalar branch (the step is the same for the whole workgroup)
          switch (__builtin_amdgcn_readfirstlane(tj))
          {
            case 1: _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = lane_xor<1>(v[e], lane); break;
            case 2: _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = lane_xor<2>(v[e], lane); break;
            case 4: _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = lane_xor<4>(v[e], lane); break;
            case 8: _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = lane_xor<8>(v[e], lane); break;
            case 16: _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = lane_xor<16>(v[e], lane); break;
            default: _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = lane_xor<32>(v[e], lane); break;
          }
        }
        else
        {
#pragma unroll
          for (int e = 0; e < 4; ++e) { sk[buf][4 * t + e] = v[e].k; si[buf][4 * t + e] = v[e].i; }
          __syncthreads();
          const int pt = t ^ tj;
#pragma unroll
          for (int e = 0; e < 4; ++e) { o[e].k = sk[buf][4 * pt + e]; o[e].i = si[buf][4 * pt + e]; }
          buf ^= 1;  // the next step through LDS writes the other buffer: this one may still be read
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
        {
          const bool up = (((4 * t + e) & k) == 0);
          const bool take_min = lower == up;
          const bool mine_gt = pair_gt(v[e], o[e]);
          if (mine_gt == take_min) v[e] = o[e];
        }
      }
    }
#pragma unroll
  for (int e = 0; e < 4; ++e)
  {
    const int i = base + 4 * t + e;
    if (i < n) { out_keys[i] = v[e].k; out_idx[i] = v[e].i; }
  }
}
// launch 4 (more than one run): every pair's place is the number of pairs of all runs in front of it
__device__ __forceinline__ void d_merge_runs(int bx, const u64* __restrict__ keys, const unsigned* __restrict__ idx, int n, u64* __restrict__ out_keys,
                                                    unsigned* __restrict__ out_idx)
{
  const int e = bx * 256 + threadIdx.x;
  if (e >= n) return;
  const u64 k = keys[e];
  const unsigned id = idx[e];
  const int mine = e / kRun;
  int rank = e - mine * kRun;
  for (int q = 0; q * kRun < n; ++q)
  {
    if (q == mine) continue;
    int lo = q * kRun, hi = min(n, (q + 1) * kRun);
    const int first = lo;
    while (lo < hi)
    {
      const int mid = (lo + hi) >> 1;
      const u64 km = keys[mid];
      if (km < k || (km == k && idx[mid] < id)) lo = mid + 1; else hi = mid;
    }
    rank += lo - first;
  }
  out_keys[rank] = k;
  out_idx[rank] = id;
}

// launch 5: one thread per place of the sorted batch; the first of a run of equal keys folds the run's points into the
// voxel, in arrival order, by the reference's per-point rule.  An existing voxel is updated where it is (the old array);
// a new one is left at the thread's own place in `fresh`, flagged, with its rank among the new ones of the block.
__device__ __forceinline__ void d_add_fold(int bx, const float4* __restrict__ batch, int n, const u64* __restrict__ skeys, const unsigned* __restrict__ sorder,
                                                  GridParams p, int* __restrict__ st, int use_box, MapView map, MapView fresh, int* __restrict__ fresh_flag,
                                                  int* __restrict__ fresh_chunks, int fixed, double time, int* __restrict__ vrank = nullptr, bool only_flags = false)
{
  __shared__ int wave_cnt[4];
  if (bx * 256 >= n) return;  // (a launch shared with a bigger batch)
  const Shift sft = roll_shift(p, st, use_box);
  const int g = p.grid_size;
  const int j0 = bx * 256 + threadIdx.x;
  const u64 key = j0 < n ? skeys[j0] : kNoKey;
  const bool head = j0 < n && key != kNoKey && (j0 == 0 || skeys[j0 - 1] != key);
  bool is_fresh = false;
  // Where the block's 256 sorted keys lie in the old array: the places of its first and of its last valid key, found by a
  // wavefront each (64 probes per round trip); every thread then searches between the two -- a few hundred voxels, a
  // handful of cache lines the block shares -- instead of the whole map.
  __shared__ int bound[2];
  const int N = st[kStN];
  {
    const int wv = threadIdx.x >> 6;
    if (wv < 2)
    {
      // the last valid key of the block: the keys ascend and the invalid ones (kNoKey) sort last
      int jl = min(n, bx * 256 + 256) - 1;
      const u64 kf = skeys[bx * 256];
      u64 kl = skeys[jl];
      int res = wv == 0 ? 0 : N;
      if (wv == 0 && kf != kNoKey) res = lower_bound_old_wave(map.keys, N, vkey_of_new(kf, sft, g), sft.any, g);
      if (wv == 1 && kl != kNoKey) res = lower_bound_old_wave(map.keys, N, vkey_of_new(kl, sft, g), sft.any, g);
      if ((threadIdx.x & 63) == 0) bound[wv] = res;
    }
    __syncthreads();
  }
  if (head)
  {
    const VKey target = vkey_of_new(key, sft, g);
    const int at = lower_bound_old_in(map.keys, bound[0], min(N, max(bound[1], bound[0])), target, sft.any, g);
    bool exists = false;
    if (at < N)
    {
      const VKey k = vkey_of_old(map.keys[at], sft.any, g);
      exists = k.hi == target.hi && k.lo == target.lo;
    }
    float4 va, vb;      // the voxel's point
    unsigned count = 0;
    bool have = exists;
    bool changed = false;
    if (exists) { va = map.pts[2 * (size_t)at]; vb = map.pts[2 * (size_t)at + 1]; count = map.count[at]; }
    else { va = make_float4(0.f, 0.f, 0.f, 0.f); vb = va; }
    // CENTER_POINT (:253): the centre is that of the leaf voxel of the point at hand, voxelGridCenterIn - VoxelResolution / 2.f
    // + LeafSize * voxelCoordIn -- two leaf voxels of one outer voxel can share an inner index (To1d of coordinates around
    // zero), so the points of one run do not all have the same centre
    float base[3] = {0.f, 0.f, 0.f};  // voxelGridCenterIn: the same for the whole run
    if (p.sampling == 3)
    {
      int id = (int)(unsigned)(key >> 32);
      const int oz = id / (g * g); id -= oz * g * g;
      const int oy = id / g; const int ox = id - oy * g;
      const int out[3] = {ox, oy, oz};
#pragma unroll
      for (int d = 0; d < 3; ++d)
      {
        const float origin = sft.pos[d] - (float)((double)(g / 2) * p.resolution_d);
        base[d] = (float)out[d] * p.resolution + origin;
      }
    }
    bool counted = false;
    // CENTROID (:263-297).  The reference keeps, per voxel that an earlier point of this Add fell into, the running mean of
    // those points -- and, INSIDE its loop over the points, pulls EVERY such voxel's point towards its mean once per point
    // of the whole cloud that gets as far as the end of the loop body ((point * count + mean) / (count + 1), :282-297).  A
    // voxel's point therefore depends on how many such points lie between and behind its own in arrival order: vrank.
    float mean[3] = {0.f, 0.f, 0.f};
    unsigned mean_count = 0;
    bool in_mean = false;
    int prev_rank = -1;
    auto pull = [&](int times) {
      const float c = (float)count, c1 = (float)(count + 1);
      for (int it = 0; it < times; ++it)
      {
        const float nx = (va.x * c + mean[0]) / c1, ny = (va.y * c + mean[1]) / c1, nz = (va.z * c + mean[2]) / c1;
        if (nx == va.x && ny == va.y && nz == va.z) break;  // a fixed point of the step: nothing moves any more
        va.x = nx; va.y = ny; va.z = nz;
      }
    };
    for (int j = j0; j < n && skeys[j] == key; ++j)
    {
      const unsigned src = sorder[j];
      const float4 a = batch[2 * (size_t)src], b = batch[2 * (size_t)src + 1];
      if (only_flags)
      {
        // (first of the CENTROID launches) does this point get to the end of the loop body?  Not when its voxel holds a
        // fixed point (:219-220) -- from before, or because an earlier point of this very call made it one
        bool through = true;
        if (!have) { have = true; vb.w = __uint_as_float((fixed ? 1u : 0u) << 24); }
        else if (((__float_as_uint(vb.w) >> 24) & 0xffu) == 1) through = false;
        else vb.w = __uint_as_float((__float_as_uint(vb.w) & 0x00ffffffu) | ((fixed ? 1u : 0u) << 24));
        vrank[src] = through ? 1 : 0;
        continue;
      }
      if (!have)
      {
        va = a; vb = b; have = true; changed = true;  // new voxel: the point as it is (:206-212)
      }
      else
      {
        const unsigned label = (__float_as_uint(vb.w) >> 24) & 0xffu;
        if (label == 1) continue;  // the voxel holds a fixed point: nothing of this point is taken, not even its time (:219-220)
        if (p.sampling == 4)
        {
          // the pulls of the points of other voxels since this voxel's last one, then this point into the mean
          if (in_mean) pull(vrank[src] - prev_rank - 1);
          const float mc = (float)mean_count, mc1 = (float)(mean_count + 1);
          mean[0] = (mean[0] * mc + a.x) / mc1; mean[1] = (mean[1] * mc + a.y) / mc1; mean[2] = (mean[2] * mc + a.z) / mc1;
          ++mean_count;
          in_mean = true;
        }
        if (p.sampling == 1) { va = a; vb = b; changed = true; }                       // LAST
        else if (p.sampling == 2) { if (b.z > vb.z) { va = a; vb = b; changed = true; } }  // MAX_INTENSITY
        else if (p.sampling == 3)
        {
          const float pt[3] = {a.x, a.y, a.z};
          float centre[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) centre[d] = base[d] - p.resolution / 2.f + p.leaf * (float)round_to_int((pt[d] - base[d]) / p.leaf);
          const float d1x = a.x - centre[0], d1y = a.y - centre[1], d1z = a.z - centre[2];
          const float d0x = va.x - centre[0], d0y = va.y - centre[1], d0z = va.z - centre[2];
          // Eigen's Vector3f norm: sqrt(x^2 + (y^2 + z^2))
          if (sqrtf(d1x * d1x + (d1y * d1y + d1z * d1z)) < sqrtf(d0x * d0x + (d0y * d0y + d0z * d0z))) { va = a; vb = b; changed = true; }
        }
      }
      if (p.sampling == 4)
      {
        if (in_mean) pull(1);  // this point's own turn of the loop at :282-297
        prev_rank = vrank[src];
      }
      // voxel.point.time = currentTime; label = fixed (:300-306); one count per Add call (:307-311)
      const long long tb = __double_as_longlong(time);
      vb.x = __int_as_float((int)(tb & 0xffffffffll));
      vb.y = __int_as_float((int)(tb >> 32));
      vb.w = __uint_as_float((__float_as_uint(vb.w) & 0x00ffffffu) | ((fixed ? 1u : 0u) << 24));
      if (!counted) { ++count; counted = true; }
    }
    if (!only_flags)
    {
    if (p.sampling == 4 && in_mean) pull(vrank[n] - prev_rank - 1);  // the points of the cloud behind this voxel's last one
    if (exists)
    {
      map.pts[2 * (size_t)at] = va;
      map.pts[2 * (size_t)at + 1] = vb;
      map.count[at] = count;
    }
    else
    {
      is_fresh = true;
      fresh.keys[j0] = key;
      fresh.pts[2 * (size_t)j0] = va;
      fresh.pts[2 * (size_t)j0 + 1] = vb;
      fresh.count[j0] = count;
    }
    if (changed) st[kStUpdated] = 1;
    }
  }
  if (only_flags)
  {
    // points outside the grid (no key) never enter the loop body
    if (j0 < n && key == kNoKey) vrank[sorder[j0]] = 0;
    return;
  }
  // rank of every place among the block's new voxels (the places that hold none get the rank the next one would)
  const u64 ballot = __ballot(is_fresh);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) wave_cnt[wv] = __popcll(ballot);
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wv; ++w) before += wave_cnt[w];
  if (j0 < n) fresh_flag[j0] = ((before + __popcll(ballot & ((1ull << lane) - 1ull))) << 1) | (is_fresh ? 1 : 0);
  if (threadIdx.x == 0) fresh_chunks[bx] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// launch 6: the new map.  Blocks [0, oblocks): 1024 old voxels each -- a survivor's place is its rank among the survivors
// plus the number of new voxels in front of it; the other blocks: 256 places of the sorted batch each -- a new voxel's
// place is its rank among the new ones plus the number of survivors in front of it.  Two forms.  kGlobal = false: every block scans
// the chunk counts of both arrays for itself (dynamic LDS: ochunks + fchunks + 2 ints) -- a keyframe's insertion: a few hundred
// entries, one launch.  kGlobal = true: the launches in front of this one have left the scans in global memory (launch_scans)
// -- an insertion whose table does not fit LDS: a long log, a prior map; no dynamic LDS.
template <bool kGlobal>
__device__ __forceinline__ void d_add_merge(int bx, GridParams p, int* __restrict__ st, int use_box, MapView old, const int* __restrict__ old_local,
                                                   const int* __restrict__ old_chunks, int ochunks, int oblocks, const u64* __restrict__ skeys, int n, MapView fresh,
                                                   const int* __restrict__ fresh_flag, const int* __restrict__ fresh_chunks, int fchunks, MapView dst,
                                                   u64* __restrict__ rec = nullptr, const unsigned* __restrict__ sorder = nullptr,
                                                   const int* __restrict__ goscan = nullptr, const int* __restrict__ gfscan = nullptr)
{
  // oblocks: where the launch's blocks for the sorted batch begin (it may be shared with a bigger map)
  if (bx < oblocks ? bx >= ochunks : (bx - oblocks) * 256 >= n) return;
  const Shift sft = roll_shift(p, st, use_box);
  const int g = p.grid_size;
  const int N = st[kStN];
  const int *oscan, *fscan;  // [ochunks + 1] exclusive scan of the survivors per chunk, [fchunks + 1] of the new voxels per block
  if constexpr (kGlobal) { oscan = goscan; fscan = gfscan; }
  else
  {
  extern __shared__ int scan[];  // the one, then the other
  __shared__ int carry;
  oscan = scan;
  fscan = scan + ochunks + 1;
  // both scans, 256 entries at a time
  for (int which = 0; which < 2; ++which)
  {
    const int* src = which ? fresh_chunks : old_chunks;
    int* out = which ? scan + ochunks + 1 : scan;
    const int cnt = which ? fchunks : ochunks;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < cnt; b0 += 256)
    {
      const int c = b0 + threadIdx.x;
      const int v = c < cnt ? src[c] : 0;
      __shared__ int wsum[4];
      const int before = carry + block_exclusive_scan<4>(v, wsum);
      if (c < cnt) out[c] = before;
      __syncthreads();
      if (threadIdx.x == 255) carry = before + v;
      __syncthreads();
    }
    if (threadIdx.x == 0) out[cnt] = carry;
    __syncthreads();
  }
  }
  const int survivors = oscan[ochunks], created = fscan[fchunks];
  if (bx == 0 && threadIdx.x == 0) { st[kStCompact] = survivors; st[kStNew] = created; }
  auto fresh_before = [&](int j) { return j >= n ? created : fscan[j >> 8] + (fresh_flag[j] >> 1); };
  auto survivors_before = [&](int i) { return i >= N ? survivors : oscan[i >> 10] + old_local[i]; };
  if ((int)bx < oblocks)
  {
    for (int q = 0; q < 4; ++q)
    {
      const int i = bx * 1024 + q * 256 + threadIdx.x;
      if (i >= N) continue;
      u64 nk;
      if (!shifted_key(old.keys[i], sft, g, nk)) continue;
      const int at = survivors_before(i) + fresh_before(lower_bound_u64(skeys, n, nk));
      dst.keys[at] = nk;
      dst.pts[2 * (size_t)at] = old.pts[2 * (size_t)i];
      dst.pts[2 * (size_t)at + 1] = old.pts[2 * (size_t)i + 1];
      dst.count[at] = old.count[i];
    }
    return;
  }
  const int j = (bx - oblocks) * 256 + threadIdx.x;
  if (j >= n || !(fresh_flag[j] & 1)) return;
  const u64 key = skeys[j];
  const int at = fresh_before(j) + survivors_before(lower_bound_old(old.keys, N, vkey_of_new(key, sft, g), sft.any, g));
  dst.keys[at] = key;
  dst.pts[2 * (size_t)at] = fresh.pts[2 * (size_t)j];
  dst.pts[2 * (size_t)at + 1] = fresh.pts[2 * (size_t)j + 1];
  dst.count[at] = fresh.count[j];
  if (rec)
  {
    // "Ordered" = 0: the new voxel's key and its first point's place in the batch (the head of its run: the run is sorted by
    // arrival), at the voxel's rank among the new ones
    const int r = fresh_before(j);
    rec[2 * (size_t)r] = key;
    rec[2 * (size_t)r + 1] = sorder[j];
  }
}
// launch 7: the move and the counts become the grid's state (Roll recounts the points when the grid moved, :155)
__device__ __forceinline__ void d_add_commit(int bx, GridParams p, int* __restrict__ st, int use_box)
{
  if (threadIdx.x != 0 || bx != 0) return;
  const Shift s = roll_shift(p, st, use_box);
  const int survivors = st[kStCompact], created = st[kStNew];
  st[kStNbPoints] = (s.any ? survivors : st[kStNbPoints]) + created;
  st[kStN] = survivors + created;
  for (int d = 0; d < 3; ++d)
  {
    st[kStOff + d] = s.off[d];
    st[kStPosX + d] = __float_as_int(s.pos[d]);
    st[kStTmp + d] = kBoxLoArmedS;            // the box is re-armed for the next batch
    st[kStTmp + 3 + d] = kBoxHiArmedS;
  }
}

// One launch of each step serves all the maps of a keyframe (blockIdx.y = map): the insertions of the keypoint types run
// side by side instead of one behind the other on the stream they share.
struct AddOne
{
  const float4* batch;
  int n, use_box, fixed;
  double time;
  GridParams p;
  int* st;
  u64 *bkeys, *skeys;
  unsigned *border, *sorder;
  MapView map, fresh, dst;
  int *old_local, *old_chunks, *fresh_flag, *fresh_chunks;
  int* vrank;
  u64* rec;  // "Ordered" = 0: {key, first arrival} of every voxel the Add creates
  int ochunks;
};
struct AddBatch
{
  AddOne a[3];
  int kblocks, oblocks;  // of the launch: the largest of the maps'
};
__global__ __launch_bounds__(256) void k_batch_bbox(AddBatch b) { const AddOne& A = b.a[blockIdx.y]; if (A.use_box) d_batch_bbox(blockIdx.x, A.batch, A.n, A.st); }
__global__ __launch_bounds__(256) void k_add_keys(AddBatch b)
{
  const AddOne& A = b.a[blockIdx.y];
  d_add_keys(blockIdx.x, A.batch, A.n, b.kblocks, A.p, A.st, A.use_box, A.bkeys, A.map.keys, A.old_local, A.old_chunks, A.ochunks);
}
__global__ __launch_bounds__(1024) void k_sort_runs(AddBatch b) { const AddOne& A = b.a[blockIdx.y]; d_sort_runs(blockIdx.x, A.bkeys, A.n, A.bkeys, A.border); }
__global__ __launch_bounds__(256) void k_merge_runs(AddBatch b) { const AddOne& A = b.a[blockIdx.y]; d_merge_runs(blockIdx.x, A.bkeys, A.border, A.n, A.skeys, A.sorder); }
__global__ __launch_bounds__(256) void k_add_fold(AddBatch b)
{
  const AddOne& A = b.a[blockIdx.y];
  d_add_fold(blockIdx.x, A.batch, A.n, A.skeys, A.sorder, A.p, A.st, A.use_box, A.map, A.fresh, A.fresh_flag, A.fresh_chunks, A.fixed, A.time, A.vrank, false);
}
// CENTROID sampling only, in front of the fold: which points of the batch get to the end of the loop body (k_add_flags: the
// fold's own walk over the runs, nothing written but the flags), and how many of them lie in front of every point in
// ARRIVAL order (k_add_vscan: exclusive scan in place, one workgroup per map; [n] = all of them)
__global__ __launch_bounds__(256) void k_add_flags(AddBatch b)
{
  const AddOne& A = b.a[blockIdx.y];
  if (A.p.sampling != 4) return;
  d_add_fold(blockIdx.x, A.batch, A.n, A.skeys, A.sorder, A.p, A.st, A.use_box, A.map, A.fresh, A.fresh_flag, A.fresh_chunks, A.fixed, A.time, A.vrank, true);
}
__global__ __launch_bounds__(1024) void k_add_vscan(AddBatch b)
{
  const AddOne& A = b.a[blockIdx.y];
  if (A.p.sampling != 4) return;
  __shared__ int s[1024];
  int run = 0;
  for (int base = 0; base < A.n; base += 1024)
  {
    const int i = base + threadIdx.x;
    const int v = i < A.n ? A.vrank[i] : 0;
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1)
    {
      const int a = threadIdx.x >= (unsigned)o ? s[threadIdx.x - o] : 0;
      __syncthreads();
      s[threadIdx.x] += a;
      __syncthreads();
    }
    if (i < A.n) A.vrank[i] = run + s[threadIdx.x] - v;
    run += s[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) A.vrank[A.n] = run;
}
__global__ __launch_bounds__(256) void k_add_merge(AddBatch b)
{
  const AddOne& A = b.a[blockIdx.y];
  d_add_merge<false>(blockIdx.x, A.p, A.st, A.use_box, A.map, A.old_local, A.old_chunks, A.ochunks, b.oblocks, A.skeys, A.n, A.fresh, A.fresh_flag, A.fresh_chunks,
                     (A.n + 255) / 256, A.dst, A.rec, A.sorder);
}

// ---- the scans of the other form, in global memory -------------------------------------------------------------------------
// A plain multi-level exclusive scan, for up to six arrays at a time (blockIdx.y: the old chunks and the batch's blocks of
// up to three maps).  A level: every block scans `per` entries (its block size) and leaves their sum; the sums are the next
// level's entries, scanned in place the same way, until one block takes them all; then, from the top level down, every entry
// gets the scanned sum of its block.  out[cnt] is the total.  A kernel boundary is the only thing a block ever waits for:
// nothing spins on another block's flag.
struct ScanLevel
{
  const int* src[6];
  int* out[6];   // (== src from the second level on)
  int* sums[6];  // [blocks + 1]
  int cnt[6];    // 0: nothing (left) to do for this array
  int per;
};
__global__ __launch_bounds__(256) void k_scan_blocks(ScanLevel L)
{
  __shared__ int wsum[4];
  const int j = blockIdx.y, cnt = L.cnt[j], per = L.per;
  if (cnt <= 0) return;
  const int nb = (cnt + per - 1) / per;
  if ((int)blockIdx.x >= nb) return;  // (a launch shared with a longer array)
  const int c = blockIdx.x * per + threadIdx.x;
  const int v = c < cnt ? L.src[j][c] : 0;
  const int before = block_exclusive_scan<4>(v, wsum);  // (the block is `per` threads: one wavefront or four)
  if (c < cnt) L.out[j][c] = before;
  if ((int)threadIdx.x == per - 1)
  {
    L.sums[j][blockIdx.x] = before + v;
    if (nb == 1) L.out[j][cnt] = before + v;
  }
}
__global__ __launch_bounds__(256) void k_scan_addback(ScanLevel L)
{
  const int j = blockIdx.y, cnt = L.cnt[j], per = L.per;
  if (cnt <= per) return;  // nothing, or one block: complete as it is
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < cnt) L.out[j][c] += L.sums[j][c / per];
  else if (c == cnt) L.out[j][cnt] = L.sums[j][(cnt + per - 1) / per];  // the scanned sums' own total
}
struct ScanPtrs
{
  const int *oscan[3], *fscan[3];
};
__global__ __launch_bounds__(256) void k_add_merge_global(AddBatch b, ScanPtrs s)
{
  const AddOne& A = b.a[blockIdx.y];
  d_add_merge<true>(blockIdx.x, A.p, A.st, A.use_box, A.map, A.old_local, A.old_chunks, A.ochunks, b.oblocks, A.skeys, A.n, A.fresh, A.fresh_flag, A.fresh_chunks,
                    (A.n + 255) / 256, A.dst, A.rec, A.sorder, s.oscan[blockIdx.y], s.fscan[blockIdx.y]);
}
struct ScanJob
{
  const int* src;
  int* out;   // [cnt + 1]; may be src
  int* sums;  // room for sums_room(cnt) ints
  int cnt;
};
size_t sums_room(int cnt) { return (size_t)cnt / 32 + 32; }  // more than the sum over the levels of (blocks + 1), with blocks of 64 entries or more
void launch_scans(hipStream_t st, const ScanJob* jobs, int nj, int per)
{
  ScanLevel lv[8];  // (64^6 entries are more than an int counts)
  int blocks[8];
  int depth = 0;
  ScanLevel cur{};
  cur.per = per;
  for (int j = 0; j < nj; ++j) { cur.src[j] = jobs[j].src; cur.out[j] = jobs[j].out; cur.sums[j] = jobs[j].sums; cur.cnt[j] = jobs[j].cnt; }
  for (;;)
  {
    ScanLevel next{};
    next.per = per;
    int most = 0;
    for (int j = 0; j < nj; ++j)
    {
      const int nb = cur.cnt[j] > 0 ? (cur.cnt[j] + per - 1) / per : 0;
      most = std::max(most, nb);
      if (nb > 1) { next.src[j] = next.out[j] = cur.sums[j]; next.sums[j] = cur.sums[j] + nb + 1; next.cnt[j] = nb; }
    }
    if (most == 0) break;
    lv[depth] = cur;
    blocks[depth++] = most;
    if (most == 1 || depth == 8) break;
    cur = next;
  }
  for (int l = 0; l < depth; ++l) hipLaunchKernelGGL(k_scan_blocks, dim3(blocks[l], nj), dim3(per), 0, st, lv[l]);
  for (int l = depth - 2; l >= 0; --l)
  {
    int most = 0;
    for (int j = 0; j < nj; ++j) most = std::max(most, lv[l].cnt[j]);
    hipLaunchKernelGGL(k_scan_addback, dim3(most / 256 + 1, nj), dim3(256), 0, st, lv[l]);
  }
}
__global__ void k_add_commit(AddBatch b) { const AddOne& A = b.a[blockIdx.y]; d_add_commit(blockIdx.x, A.p, A.st, A.use_box); }
}  // namespace

namespace lsa
{
int ensure_batch(lsa_device_grid* g, int n)
{
  if (n <= g->bcap) return LSA_OK;
  // (twice what is asked for: outgrowing the batch retires eight buffers, and freeing them at the next frame's start waits for
  //  the device eight times -- 0.2-0.6 ms; a keyframe's keypoint count wanders by a quarter over the first hundred frames)
  const int cap = (int)std::min(std::max(2ll * n, 1ll << 15), kAddressable);
  auto fr = [g](void* p) { retire_dev(g->ctx, p); };
  fr(g->batch); fr(g->bkeys); fr(g->skeys); fr(g->border); fr(g->sorder); fr(g->heads); fr(g->fresh_flag); fr(g->vrank);
  retire_view(g, g->fresh);
  G_HIP(hipMalloc((void**)&g->batch, (size_t)cap * 2 * sizeof(float4)));
  G_HIP(hipMalloc((void**)&g->bkeys, (size_t)cap * sizeof(u64)));
  G_HIP(hipMalloc((void**)&g->skeys, (size_t)cap * sizeof(u64)));
  G_HIP(hipMalloc((void**)&g->border, (size_t)cap * sizeof(unsigned)));
  G_HIP(hipMalloc((void**)&g->sorder, (size_t)cap * sizeof(unsigned)));
  G_HIP(hipMalloc((void**)&g->heads, (size_t)cap * sizeof(int)));
  G_HIP(hipMalloc((void**)&g->fresh_flag, (size_t)cap * sizeof(int)));
  G_HIP(hipMalloc((void**)&g->vrank, ((size_t)cap + 1) * sizeof(int)));
  int rc = alloc_view(g, g->fresh, cap);
  if (rc) return rc;
  g->bcap = cap;
  return LSA_OK;
}

// room for the scans of the form that keeps them in global memory: grown like the batch scratch, nothing freed while work may be
// in flight
static int ensure_scans(lsa_device_grid* g, int ochunks, int fchunks, size_t sums)
{
  auto grow = [g](int*& p, int& cap, size_t want) -> int {
    if (want <= (size_t)cap) return LSA_OK;
    const size_t to = std::min<size_t>(std::max<size_t>(2 * want, 1 << 12), 0x7fffffff);
    retire_dev(g->ctx, p);
    p = nullptr;
    cap = 0;
    G_HIP(hipMalloc((void**)&p, to * sizeof(int)));
    cap = (int)to;
    return LSA_OK;
  };
  int rc = grow(g->oscan, g->oscan_cap, (size_t)ochunks + 1);
  if (!rc) rc = grow(g->fscan, g->fscan_cap, (size_t)fchunks + 1);
  if (!rc) rc = grow(g->scan_sums, g->scan_sums_cap, sums);
  return rc;
}

// Add of the ns[i] points in gs[i]->batch (device), for up to three maps of one context at a time: seven launches
// whatever the number of maps -- while the chunk tables of the merge fit LDS (every keyframe's do); a few more for the scans in
// global memory when they do not, or when a map's "GlobalScans" asks for that form
int add_batches(lsa_device_grid* const* gs, const int* ns, int count, bool fixed, double time, bool do_roll)
{
  lsa_device_grid* g = gs[0];  // (for the error macro; all maps share the context and the stream)
  hipStream_t st = g->stream;
  AddBatch b{};
  int kmax = 0, omax = 0, runs = 0;
  for (int i = 0; i < count; ++i)
  {
    lsa_device_grid* gi = gs[i];
    if (gi->ctx != g->ctx || gi->stream != st) return g->ctx->fail(LSA_E_ARG, "lsa_device_grid: the maps of one insertion share a context");
    tighten(gi);
    if ((long long)gi->n_upper + ns[i] > kAddressable)
      return g->ctx->fail(LSA_E_CAPACITY, "lsa_device_grid: the voxels of the map (" + std::to_string(gi->n_upper) + ") and the points of the insertion (" + std::to_string(ns[i]) +
                                              ") together are more than one insertion addresses (2^31 - 8193)");
    const int rc = begin_modification(gi, gi->n_upper + ns[i], 2 * (size_t)ns[i]);
    if (rc) return rc;
    AddOne& A = b.a[i];
    A.batch = gi->batch; A.n = ns[i]; A.use_box = do_roll ? 1 : 0; A.fixed = fixed ? 1 : 0; A.time = time;
    A.p = params_of(gi); A.st = gi->st;
    A.bkeys = gi->bkeys; A.skeys = gi->skeys; A.border = gi->border; A.sorder = gi->sorder;
    A.map = gi->buf[gi->cur]; A.dst = gi->buf[1 - gi->cur]; A.fresh = gi->fresh;
    A.old_local = gi->old_local; A.old_chunks = gi->chunks; A.fresh_flag = gi->fresh_flag; A.fresh_chunks = gi->heads; A.vrank = gi->vrank;
    A.rec = gi->Ordered ? nullptr : gi->rec_dev;
    A.ochunks = std::max((gi->n_upper + 1023) / 1024, 1);
    kmax = std::max(kmax, (ns[i] + 255) / 256);
    omax = std::max(omax, A.ochunks);
    runs = std::max(runs, (ns[i] + kRun - 1) / kRun);
  }
  b.kblocks = kmax;
  b.oblocks = omax;
  const size_t lds = (size_t)(omax + kmax + 2) * sizeof(int);
  // the form: the tables in LDS while they fit (12 288 entries: n / 256 + voxels / 1024), in global memory otherwise
  int knob = 0;
  for (int i = 0; i < count; ++i) knob = std::max(knob, gs[i]->GlobalScans);
  const bool global = knob != 0 || lds > 48 * 1024;
  const int per = knob == 2 ? 64 : 256;  // entries a scan block takes
  ScanJob tables[6], flags[3];
  ScanPtrs sp{};
  if (global)
    for (int i = 0; i < count; ++i)
    {
      lsa_device_grid* gi = gs[i];
      const int fchunks = (ns[i] + 255) / 256, ochunks = b.a[i].ochunks;
      // the block sums: of the flags of CENTROID first, then (the flags' scan is over) of the two tables side by side
      const int rc = ensure_scans(gi, ochunks, fchunks, std::max(sums_room(ns[i]), sums_room(ochunks) + sums_room(fchunks)));
      if (rc) return rc;
      tables[2 * i] = ScanJob{gi->chunks, gi->oscan, gi->scan_sums, ochunks};
      tables[2 * i + 1] = ScanJob{gi->heads, gi->fscan, gi->scan_sums + sums_room(ochunks), fchunks};
      flags[i] = ScanJob{gi->vrank, gi->vrank, gi->scan_sums, b.a[i].p.sampling == 4 ? ns[i] : 0};
      sp.oscan[i] = gi->oscan;
      sp.fscan[i] = gi->fscan;
    }
  double bytes = 0;
  for (int i = 0; i < count; ++i) bytes += (double)ns[i] * (32 + 12 + 44) + (double)gs[i]->n_upper * 44 * 2;
  {
    ProfScope ps(g->ctx, "map_add", bytes, st);
    const unsigned y = (unsigned)count;
    if (do_roll) hipLaunchKernelGGL(k_batch_bbox, dim3(kmax, y), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_add_keys, dim3(kmax + omax, y), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_sort_runs, dim3(runs, y), dim3(1024), 0, st, b);
    hipLaunchKernelGGL(k_merge_runs, dim3(kmax, y), dim3(256), 0, st, b);
    bool centroid = false;
    for (int i = 0; i < count; ++i) centroid = centroid || b.a[i].p.sampling == 4;
    if (centroid)
    {
      hipLaunchKernelGGL(k_add_flags, dim3(kmax, y), dim3(256), 0, st, b);
      // (one workgroup per map walks the whole batch: linear, but alone -- 10 ms for three million points; the multi-level scan instead)
      if (global) launch_scans(st, flags, count, per);
      else hipLaunchKernelGGL(k_add_vscan, dim3(1, y), dim3(1024), 0, st, b);
    }
    hipLaunchKernelGGL(k_add_fold, dim3(kmax, y), dim3(256), 0, st, b);
    if (global)
    {
      launch_scans(st, tables, 2 * count, per);
      hipLaunchKernelGGL(k_add_merge_global, dim3(omax + kmax, y), dim3(256), 0, st, b, sp);
    }
    else hipLaunchKernelGGL(k_add_merge, dim3(omax + kmax, y), dim3(256), lds, st, b);
    hipLaunchKernelGGL(k_add_commit, dim3(1, y), dim3(64), 0, st, b);
  }
  for (int i = 0; i < count; ++i)
  {
    gs[i]->cur = 1 - gs[i]->cur;
    gs[i]->n_upper += ns[i];
    // (whether a point changed -- the kd-tree is only dropped then, :315-317 -- is read by lsa_device_grid_submap_valid)
    const int rc = end_modification(gs[i], kRecAdd, 2 * (size_t)ns[i]);
    if (rc) return rc;
  }
  return LSA_OK;
}

// ---- what lsa_pcd.hip and lsa_kplog.hip need of an insertion (lsa_device_grid_io.h) ----
// room for a batch of n points: the buffer a conversion kernel on the grid's stream fills before grid_add_batch(n)
int grid_batch(lsa_device_grid* g, int n, lsa_point_t** batch)
{
  G_HIP(hipSetDevice(g->ctx->device));
  const int rc = ensure_batch(g, n);
  if (rc) return rc;
  g->staged = 0;
  *batch = reinterpret_cast<lsa_point_t*>(g->batch);
  return LSA_OK;
}
int grid_add_batch(lsa_device_grid* g, int n, bool fixed, double time, bool do_roll) { return add_batches(&g, &n, 1, fixed, time, do_roll); }
}  // namespace lsa

extern "C" {

int lsa_device_grid_add(lsa_device_grid* g, const lsa_point_t* pts, int n, int fixed, double time, int roll_first)
{
  if (!g || n < 0 || (!pts && n > 0)) return g ? g->ctx->fail(LSA_E_ARG, "lsa_device_grid_add: bad argument") : LSA_E_ARG;
  if (n == 0) return LSA_OK;  // "Pointcloud is empty, voxel grid not updated."
  G_HIP(hipSetDevice(g->ctx->device));
  int rc = ensure_batch(g, n);
  if (rc) return rc;
  G_HIP(hipMemcpyAsync(g->batch, pts, (size_t)n * sizeof(lsa_point_t), hipMemcpyHostToDevice, g->stream));
  G_HIP(hipStreamSynchronize(g->stream));  // pts may be pageable and go away
  return grid_add_batch(g, n, fixed != 0, time, roll_first != 0);
}

// the keypoints of a device set, moved by `pose` (WORLD), added without leaving the device: Slam::UpdateMapsUsingTworld
// (slam_lib/src/Slam.cxx:1178-1222).  In two steps for callers that hand the insertion to another host thread: _stage
// reads the context's keypoints (ordered behind what the context's stream has enqueued, and the context's stream behind
// it: the set may be rewritten right after), _add_staged is the insertion proper, on the grid's stream alone.
int lsa_device_grid_stage_keypoints(lsa_device_grid* g, int set, int type, const double pose[16])
{
  if (!g || !pose || set < 0 || set > 2 || type < 0 || type > 2) return g ? g->ctx->fail(LSA_E_ARG, "lsa_device_grid_stage_keypoints: bad argument") : LSA_E_ARG;
  lsa_ctx* ctx = g->ctx;
  const int n = ctx->kp_n[set][type];
  g->staged = 0;
  if (n <= 0) return LSA_OK;
  G_HIP(hipSetDevice(ctx->device));
  int rc = ensure_batch(g, n);
  if (rc) return rc;
  // the transform runs on the context's stream, in order with whatever rewrites the keypoints next (a few microseconds
  // on a stream that is idle at the end of a frame); the grid's stream only waits for it.  The batch buffer is free: the
  // last insertion that read it is over (ev_out, recorded behind every insertion).
  G_HIP(hipStreamWaitEvent(ctx->stream, g->ev_out, 0));
  rc = transform_points_to(ctx, ctx->kp[set][type], n, pose, reinterpret_cast<lsa_point_t*>(g->batch), ctx->stream);
  if (rc) return rc;
  g->staged = n;
  return order_after_context(g);
}
// ... of the keypoint types of a keyframe together: ONE transform launch for all the maps (a block row each), one event
int lsa_device_grid_stage_keypoints_all(lsa_device_grid* const* grids, const int* types, int count, int set, const double pose[16])
{
  if (!grids || !types || !pose || count < 1 || count > 3 || set < 0 || set > 2) return LSA_E_ARG;
  for (int i = 0; i < count; ++i)
    if (!grids[i] || types[i] < 0 || types[i] > 2 || grids[i]->ctx != grids[0]->ctx) return LSA_E_ARG;
  lsa_device_grid* g = grids[0];
  lsa_ctx* ctx = g->ctx;
  G_HIP(hipSetDevice(ctx->device));
  const lsa_point_t* src[3] = {nullptr, nullptr, nullptr};
  lsa_point_t* dst[3] = {nullptr, nullptr, nullptr};
  int ns[3] = {0, 0, 0};
  bool any = false;
  for (int i = 0; i < count; ++i)
  {
    lsa_device_grid* gi = grids[i];
    const int n = ctx->kp_n[set][types[i]];
    gi->staged = 0;
    if (n <= 0) continue;
    const int rc = ensure_batch(gi, n);
    if (rc) return rc;
    // (the batch buffer is free once the last insertion that read it is over: ev_out)
    G_HIP(hipStreamWaitEvent(ctx->stream, gi->ev_out, 0));
    src[i] = ctx->kp[set][types[i]];
    dst[i] = reinterpret_cast<lsa_point_t*>(gi->batch);
    ns[i] = n;
    any = true;
  }
  if (!any) return LSA_OK;
  const int rc = transform_sets_to(ctx, src, ns, pose, dst, ctx->stream);
  if (rc) return rc;
  G_HIP(hipEventRecord(g->ev_in, ctx->stream));
  for (int i = 0; i < count; ++i)
  {
    grids[i]->staged = ns[i];
    if (ns[i] > 0) G_HIP(hipStreamWaitEvent(grids[i]->stream, g->ev_in, 0));
  }
  return LSA_OK;
}
int lsa_device_grid_add_staged(lsa_device_grid* g, double time) { return lsa_device_grid_add_staged_all(&g, 1, time); }
// ... of several maps of one context at once (the keypoint types of a keyframe): one launch of every step for all of them
int lsa_device_grid_add_staged_all(lsa_device_grid* const* grids, int count, double time)
{
  if (!grids || count < 1 || count > 3) return LSA_E_ARG;
  lsa_device_grid* gs[3];
  int ns[3], m = 0;
  for (int i = 0; i < count; ++i)
  {
    if (!grids[i]) return LSA_E_ARG;
    if (grids[i]->staged > 0) { gs[m] = grids[i]; ns[m] = grids[i]->staged; ++m; }  // "Pointcloud is empty, voxel grid not updated."
    grids[i]->staged = 0;
  }
  if (m == 0) return LSA_OK;
  if (hipSetDevice(gs[0]->ctx->device) != hipSuccess) return LSA_E_HIP;
  return add_batches(gs, ns, m, false, time, true);
}
int lsa_device_grid_add_keypoints(lsa_device_grid* g, int set, int type, const double pose[16], double time)
{
  const int rc = lsa_device_grid_stage_keypoints(g, set, type, pose);
  return rc ? rc : lsa_device_grid_add_staged(g, time);
}

}  // extern "C"
