// lsa_scan_descriptor.h -- the polar height descriptor of a frame of keypoints and the distance between two of them, ONE
// source for the host statement (host/lsa_place.cpp) and the device (lsa_place.hip): place recognition on the keypoint log
// (DESIGN.md 3.8).  The descriptor is Scan Context's (Kim & Kim, IROS 2018): rings x sectors cells around the sensor, each
// the largest height seen in it, compared column by column under every column shift; the shift of the best match is the yaw
// between the two frames.
// Every decision -- which cell a point falls into, what a cell holds, the order of every float sum -- is taken by the text
// below on both sides.  Plain C++ (no HIP header, no libm): the angle is lsa_pmath.h's lsa_atan2, sqrt and / are the IEEE
// ones on both sides, nothing may be contracted or re-associated (-ffp-contract=off), so the same points give the same
// bits wherever this is compiled.
#pragma once
#include "../../include/lidarslam_amd.h"
#include "../../include/lsa_pmath.h"

#if defined(__HIPCC__)
#define LSA_HDP __host__ __device__ inline
#else
#define LSA_HDP inline
#endif

namespace lsa
{
namespace place
{
constexpr int kMaxRings = 32;
constexpr int kMaxSectors = 120;

// the constraints of lsa_place_params_t (include/lidarslam_amd.h)
LSA_HDP bool params_ok(const lsa_place_params_t& p)
{
  if (p.rings < 1 || p.rings > kMaxRings || p.sectors < 1 || p.sectors > kMaxSectors) return false;
  if (p.type_mask == 0u || (p.type_mask & ~7u)) return false;
  const double span = p.max_range - p.min_range;
  if (!(span > 0.) || !(span <= 1.7976931348623157e308)) return false;  // greater than min_range, both finite
  if (!(p.height_offset - p.height_offset == 0.)) return false;         // finite
  return true;
}
// min_common_sectors <= 0: the default of the shape, max(1, sectors / 4)
LSA_HDP int min_common(const lsa_place_params_t& p)
{
  if (p.min_common_sectors > 0) return p.min_common_sectors;
  return p.sectors / 4 > 1 ? p.sectors / 4 : 1;
}
LSA_HDP int cells(const lsa_place_params_t& p) { return p.rings * p.sectors; }
LSA_HDP int length(const lsa_place_params_t& p) { return p.rings * p.sectors + p.sectors; }  // floats: the cells, then the column norms

// The cell (ring * sectors + sector) of a point in the frame's own coordinates; false: the point takes no part.
LSA_HDP bool cell_of(const lsa_place_params_t& p, float x, float y, float z, int* cell)
{
  if (x != x || y != y || z != z) return false;
  const double PI = 3.14159265358979311600e+00, TWO_PI = 6.28318530717958623200e+00;
  const double r = __builtin_sqrt((double)x * (double)x + (double)y * (double)y);
  if (!(p.min_range <= r && r < p.max_range)) return false;
  int ring = (int)((r - p.min_range) / (p.max_range - p.min_range) * p.rings);
  if (ring > p.rings - 1) ring = p.rings - 1;
  const double theta = lsa_atan2((double)y, (double)x);
  int sector = (int)((theta + PI) / TWO_PI * p.sectors);
  if (sector > p.sectors - 1) sector = p.sectors - 1;
  if (sector < 0) sector = 0;
  *cell = ring * p.sectors + sector;
  return true;
}
// what a point offers to its cell, and what the cell holds in the end given the largest offer (an empty cell: 0)
LSA_HDP float offer(const lsa_place_params_t& p, float z) { return z + (float)p.height_offset; }
LSA_HDP float cell_value(float largest) { return largest > 0.f ? largest : 0.f; }
// the norm of column j: sqrtf of the float sum, rings ascending, of the squares
LSA_HDP float column_norm(const float* cellsOf, int rings, int sectors, int j)
{
  float sum = 0.f;
  for (int ring = 0; ring < rings; ++ring) sum += cellsOf[ring * sectors + j] * cellsOf[ring * sectors + j];
  return __builtin_sqrtf(sum);
}
// the cosine of column j of q and column k of c (both norms > 0): the dot over the rings ascending, one division
LSA_HDP float cosine(const float* q, const float* c, int rings, int sectors, int j, int k, float nqj, float nck)
{
  float dot = 0.f;
  for (int ring = 0; ring < rings; ++ring) dot += q[ring * sectors + j] * c[ring * sectors + k];
  return dot / (nqj * nck);
}
// the distance under one shift, from the sum of the cosines of its `cnt` common columns
LSA_HDP float shift_distance(float sum, int cnt, int minCommon) { return cnt >= minCommon ? 1.f - sum / (float)cnt : 1.f; }
// (d2, s2) beats (d, s): smaller, or as small at a lower shift
LSA_HDP bool beats(float d2, int s2, float d, int s) { return d2 < d || (d2 == d && s2 < s); }
// the yaw of a shift, in (-pi, pi]: a query taken at the candidate's place with the base turned by +yaw about z
LSA_HDP double yaw_of(int shift, int sectors)
{
  const double PI = 3.14159265358979311600e+00, TWO_PI = 6.28318530717958623200e+00;
  const double yaw = shift * TWO_PI / sectors;
  return yaw > PI ? yaw - TWO_PI : yaw;
}

// ---- the map as seen from a viewpoint -------------------------------------------------------------------------
// A viewpoint is a position v in the maps' frame, its axes the maps' axes: the base is assumed LEVEL there (roll and pitch
// are ignored -- a limit of the definition).  A map point p takes part as the frame point (map_coord(p.x, v.x), map_coord(p.y,
// v.y), map_coord(p.z, v.z)); cell_of, offer, cell_value and column_norm then apply verbatim, so the descriptor of the map at
// v is the frame descriptor of the translated points.
LSA_HDP float map_coord(float p, double v) { return (float)((double)p - v); }
// What a slice of map points whose xy box is [lo, hi] can be passed over by, and a point be dropped by before the square
// root: the planar distance the text above can still accept, with a margin.  The translation rounds to float, |x - x_true|
// <= 2^-24 |x_true|, so cell_of's r is at least d_true (1 - 2^-23) for a point at the true planar distance d_true; a point
// (or a box) farther than max_range (1 + 2^-20) therefore has r > max_range and takes no part -- sixteen times the rounding,
// which also covers the double arithmetic of the comparison itself.  max_range <= 0 accepts nothing: reach 0.
LSA_HDP double map_reach(const lsa_place_params_t& p) { return p.max_range > 0. ? p.max_range * (1. + 9.5367431640625e-07) : 0.; }
// the squared planar distance from v to the box (0 inside); an empty box (lo > hi) is infinitely far
LSA_HDP double map_box_distance2(float lox, float loy, float hix, float hiy, double vx, double vy)
{
  double dx = (double)lox - vx > vx - (double)hix ? (double)lox - vx : vx - (double)hix;
  double dy = (double)loy - vy > vy - (double)hiy ? (double)loy - vy : vy - (double)hiy;
  if (!(dx > 0.)) dx = 0.;
  if (!(dy > 0.)) dy = 0.;
  return dx * dx + dy * dy;
}
}  // namespace place
}  // namespace lsa
