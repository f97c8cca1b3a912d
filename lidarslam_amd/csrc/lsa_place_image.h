// lsa_place_image.h -- from points to a descriptor on the device (device-only; the definition is lsa_scan_descriptor.h): the
// image of the cells as words in the order-preserving coding of floats (f2ou), 0 = no point yet (no float codes to 0 but a
// NaN, and a NaN takes no part), so the largest offer of a cell is one atomic max per point whatever the order; and the
// finish, words -> cell values -> column norms.  k_log_describe (lsa_place.hip), k_map_describe and k_map_finish
// (lsa_map_place.hip) decide only where the image lives.
#pragma once
#include "lsa_scan_descriptor.h"
#include "lsa_wave.h"

namespace lsa
{
constexpr int kImageCells = place::kMaxRings * place::kMaxSectors;

// the point (x, y, z), in the frame's own coordinates, into an LDS image
__device__ __forceinline__ void image_offer(unsigned* img, const lsa_place_params_t& p, float x, float y, float z)
{
  int cell;
  if (place::cell_of(p, x, y, z, &cell)) atomicMax(&img[cell], f2ou(place::offer(p, z)));
}

// EVERY thread of the workgroup (THREADS of them) must call it, the image complete behind a barrier.  A thread per cell turns
// the word into the cell's value, writes it to the slot `out` and leaves it in LDS as a float for the norms: a lane per
// sector, rings ascending.  vals may be the words themselves (in place: the thread that reads word c writes float c).
template <int THREADS>
__device__ __forceinline__ void image_finish(const unsigned* words, float* vals, float* __restrict__ out, const lsa_place_params_t& p)
{
  const int cells = p.rings * p.sectors;
  for (int c = threadIdx.x; c < cells; c += THREADS)
  {
    const unsigned u = words[c];
    const float v = u ? place::cell_value(ou2f(u)) : 0.f;
    out[c] = v;
    vals[c] = v;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < p.sectors; j += THREADS) out[cells + j] = place::column_norm(vals, p.rings, p.sectors, j);
}
}  // namespace lsa
