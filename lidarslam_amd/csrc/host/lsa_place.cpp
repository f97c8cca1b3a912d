// lsa_place.cpp -- the host statement of place recognition (lsa_place.h) and its C ABI.
#include "lsa_place.h"
#include <cmath>
#include <cstring>
#include <vector>

namespace lsa
{
namespace host
{

int ScanDescriptor(const lsa_place_params_t& p, const lsa_point_t* pts, int n, float* out)
{
  if (!place::params_ok(p) || !out || n < 0 || (n > 0 && !pts)) return LSA_E_ARG;
  const int cells = place::cells(p);
  // the largest offer of every cell; `seen` tells an empty cell from one whose largest offer is not positive (both end as 0)
  std::vector<char> seen(static_cast<size_t>(cells), 0);
  for (int c = 0; c < cells; ++c) out[c] = 0.f;
  for (int i = 0; i < n; ++i)
  {
    int cell;
    if (!place::cell_of(p, pts[i].x, pts[i].y, pts[i].z, &cell)) continue;
    const float v = place::offer(p, pts[i].z);
    if (!seen[cell] || v > out[cell]) out[cell] = v;
    seen[cell] = 1;
  }
  for (int c = 0; c < cells; ++c) out[c] = place::cell_value(out[c]);
  for (int j = 0; j < p.sectors; ++j) out[cells + j] = place::column_norm(out, p.rings, p.sectors, j);
  return LSA_OK;
}

int PlaceDistance(const lsa_place_params_t& p, const float* a, const float* b, float* distance, int* shift)
{
  if (!place::params_ok(p) || !a || !b || !distance || !shift) return LSA_E_ARG;
  const int sectors = p.sectors, rings = p.rings, minCommon = place::min_common(p);
  const float* na = a + place::cells(p);
  const float* nb = b + place::cells(p);
  float best = 0.f;
  int bestShift = -1;
  for (int s = 0; s < sectors; ++s)
  {
    float sum = 0.f;
    int cnt = 0;
    for (int j = 0; j < sectors; ++j)
    {
      const int k = (j + s) % sectors;
      if (na[j] > 0.f && nb[k] > 0.f)
      {
        sum += place::cosine(a, b, rings, sectors, j, k, na[j], nb[k]);
        ++cnt;
      }
    }
    const float d = place::shift_distance(sum, cnt, minCommon);
    if (bestShift < 0 || place::beats(d, s, best, bestShift)) { best = d; bestShift = s; }
  }
  *distance = best;
  *shift = bestShift;
  return LSA_OK;
}

int PlaceSelect(const float* distance, const int32_t* shift, const double* poses17, int n, int query, int sectors, double minTravelled, double maxDistance,
                double maxDescriptorDistance, int exclusionHalfWindow, lsa_place_candidate_t* out, int capacity)
{
  if (!poses17 || n < 1 || query < 0 || query >= n || sectors < 1 || sectors > place::kMaxSectors || !(minTravelled >= 0.) || exclusionHalfWindow < 0 || capacity < 0 ||
      (capacity > 0 && !out) || (query > 0 && (!distance || !shift)) || maxDistance != maxDistance || maxDescriptorDistance != maxDescriptorDistance)
    return LSA_E_ARG;
  auto position = [&](int i, int d) { return poses17[17 * static_cast<size_t>(i) + 4 * d + 3]; };
  auto metres = [&](int a, int b) {
    const double dx = position(a, 0) - position(b, 0), dy = position(a, 1) - position(b, 1), dz = position(a, 2) - position(b, 2);
    return std::sqrt(dx * dx + dy * dy + dz * dz);
  };
  // travelled[i]: the way from frame 0 to frame i (LoopClosureCandidate's rule, lsa_loop_closure.h)
  std::vector<double> travelled(static_cast<size_t>(query) + 1, 0.);
  for (int i = 1; i <= query; ++i) travelled[i] = travelled[i - 1] + metres(i, i - 1);
  std::vector<char> eligible(static_cast<size_t>(query), 0);
  for (int i = 0; i < query; ++i)
  {
    if (!(travelled[query] - travelled[i] >= minTravelled)) continue;
    if (maxDistance > 0. && !(metres(i, query) <= maxDistance)) continue;
    if (maxDescriptorDistance > 0. && !(static_cast<double>(distance[i]) <= maxDescriptorDistance)) continue;
    if (distance[i] != distance[i]) continue;  // (a NaN has no rank)
    eligible[i] = 1;
  }
  int found = 0;
  while (found < capacity)
  {
    int best = -1;
    for (int i = 0; i < query; ++i)
      if (eligible[i] && (best < 0 || distance[i] < distance[best])) best = i;  // ascending: the lower index on a tie
    if (best < 0) break;
    lsa_place_candidate_t c;
    std::memset(&c, 0, sizeof(c));
    c.frame = best;
    c.shift = shift[best];
    c.distance = distance[best];
    c.yaw = place::yaw_of(shift[best], sectors);
    out[found++] = c;
    const long long lo = static_cast<long long>(best) - exclusionHalfWindow, hi = static_cast<long long>(best) + exclusionHalfWindow;
    for (long long i = lo < 0 ? 0 : lo; i <= hi && i < query; ++i) eligible[static_cast<size_t>(i)] = 0;
  }
  return found;
}

int DetectQueries(const lsa_loop_detect_t& detect, int n, int capacity, int* last)
{
  if (!place::search_ok(detect.search) || detect.per_query < 1 || detect.per_query > place::kMaxPerQuery || capacity < 0) return LSA_E_ARG;
  if (!place::query_set_ok(n, detect.first_query, detect.last_query, detect.query_stride, last)) return LSA_E_ARG;
  const int queries = place::query_count(detect.first_query, *last, detect.query_stride);
  if (static_cast<long long>(capacity) < static_cast<long long>(queries) * detect.per_query) return LSA_E_ARG;
  return queries;
}

void FramePositions(const double* poses17, int n, place::FramePosition* out)
{
  for (int i = 0; i < n; ++i)
  {
    const double* m = poses17 + 17 * static_cast<size_t>(i);
    out[i] = place::FramePosition{m[3], m[7], m[11], 0.};
    if (i > 0) out[i].travelled = out[i - 1].travelled + place::metres(out[i], out[i - 1]);
  }
}

int PlaceDetect(const lsa_loop_detect_t& detect, const float* descriptors, const double* poses17, int n, lsa_loop_candidate_t* out, int capacity)
{
  int last = 0;
  const int queries = DetectQueries(detect, n, capacity, &last);
  if (queries < 0 || !descriptors || !poses17 || !out) return LSA_E_ARG;
  const lsa_place_search_t& s = detect.search;
  const size_t length = static_cast<size_t>(place::length(s.descriptor));
  std::vector<float> distance;
  std::vector<int32_t> shift;
  lsa_place_candidate_t picked[place::kMaxPerQuery];
  int found = 0;
  for (int q = detect.first_query; q <= last; q += detect.query_stride)
  {
    distance.resize(static_cast<size_t>(q));
    shift.resize(static_cast<size_t>(q));
    for (int i = 0; i < q; ++i)
    {
      int sh = 0;
      if (PlaceDistance(s.descriptor, descriptors + length * q, descriptors + length * i, &distance[i], &sh) != LSA_OK) return LSA_E_ARG;
      shift[i] = sh;
    }
    const int got = PlaceSelect(distance.data(), shift.data(), poses17, n, q, s.descriptor.sectors, s.min_travelled, s.max_distance, s.max_descriptor_distance,
                                s.exclusion_half_window, picked, detect.per_query);
    if (got < 0) return got;
    for (int k = 0; k < got; ++k)
    {
      lsa_loop_candidate_t c;
      std::memset(&c, 0, sizeof(c));
      c.query = q;
      c.frame = picked[k].frame;
      c.shift = picked[k].shift;
      c.distance = picked[k].distance;
      c.yaw = picked[k].yaw;
      out[found++] = c;
    }
    if (q > last - detect.query_stride) break;  // (q + stride may not be an int)
  }
  return found;
}

int MapDescriptor(const lsa_place_params_t& p, const lsa_point_t* pts, int n, const double viewpoint[3], float* out)
{
  if (!place::params_ok(p) || !out || n < 0 || (n > 0 && !pts) || !viewpoint) return LSA_E_ARG;
  for (int d = 0; d < 3; ++d)
    if (!(viewpoint[d] - viewpoint[d] == 0.)) return LSA_E_ARG;
  // the definition, literally: the frame descriptor of the translated points
  std::vector<lsa_point_t> moved(pts, pts + n);
  for (lsa_point_t& q : moved)
  {
    q.x = place::map_coord(q.x, viewpoint[0]);
    q.y = place::map_coord(q.y, viewpoint[1]);
    q.z = place::map_coord(q.z, viewpoint[2]);
  }
  return ScanDescriptor(p, moved.data(), n, out);
}

bool MapSearchOk(const lsa_map_place_search_t& s)
{
  auto finite = [](double v) { return v - v == 0.; };
  if (!place::params_ok(s.descriptor) || !finite(s.max_descriptor_distance) || !finite(s.exclusion_radius) || !finite(s.max_distance)) return false;
  if (s.max_distance > 0. && !(finite(s.near_xyz[0]) && finite(s.near_xyz[1]) && finite(s.near_xyz[2]))) return false;
  return true;
}

int MapPlaceSelect(const float* distance, const int32_t* shift, const double* viewpoints, int V, int sectors, const lsa_map_place_search_t& s,
                   lsa_map_place_candidate_t* out, int capacity)
{
  if (!distance || !shift || !viewpoints || V < 1 || sectors < 1 || sectors > place::kMaxSectors || capacity < 0 || (capacity > 0 && !out) || !MapSearchOk(s))
    return LSA_E_ARG;
  for (size_t i = 0; i < 3 * static_cast<size_t>(V); ++i)
    if (!(viewpoints[i] - viewpoints[i] == 0.)) return LSA_E_ARG;
  auto metres = [&](const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz);
  };
  std::vector<char> eligible(static_cast<size_t>(V), 0);
  for (int i = 0; i < V; ++i)
  {
    if (distance[i] != distance[i]) continue;  // (a NaN has no rank)
    if (s.max_descriptor_distance > 0. && !(static_cast<double>(distance[i]) <= s.max_descriptor_distance)) continue;
    if (s.max_distance > 0. && !(metres(viewpoints + 3 * static_cast<size_t>(i), s.near_xyz) <= s.max_distance)) continue;
    eligible[i] = 1;
  }
  int found = 0;
  while (found < capacity)
  {
    int best = -1;
    for (int i = 0; i < V; ++i)
      if (eligible[i] && (best < 0 || distance[i] < distance[best])) best = i;  // ascending: the lower index on a tie
    if (best < 0) break;
    const double* v = viewpoints + 3 * static_cast<size_t>(best);
    lsa_map_place_candidate_t c;
    std::memset(&c, 0, sizeof(c));
    c.viewpoint = best;
    c.shift = shift[best];
    c.distance = distance[best];
    c.yaw = place::yaw_of(shift[best], sectors);
    const double cy = std::cos(c.yaw), sy = std::sin(c.yaw);
    const double guess[16] = {cy, -sy, 0., v[0], sy, cy, 0., v[1], 0., 0., 1., v[2], 0., 0., 0., 1.};  // Translation(v) * Rz(yaw)
    std::memcpy(c.guess, guess, sizeof(guess));
    out[found++] = c;
    eligible[best] = 0;
    if (s.exclusion_radius > 0.)
      for (int i = 0; i < V; ++i)
        if (eligible[i] && metres(viewpoints + 3 * static_cast<size_t>(i), v) <= s.exclusion_radius) eligible[i] = 0;
  }
  return found;
}

}  // namespace host
}  // namespace lsa

extern "C" {

void lsa_place_params_init(lsa_place_params_t* params)
{
  if (!params) return;
  std::memset(params, 0, sizeof(*params));
  params->rings = 20;
  params->sectors = 60;
  params->type_mask = (1u << LSA_EDGE) | (1u << LSA_PLANE);
  params->min_common_sectors = 15;
  params->min_range = 0.;
  params->max_range = 80.;
  params->height_offset = 2.;
}

void lsa_place_search_init(lsa_place_search_t* search)
{
  if (!search) return;
  std::memset(search, 0, sizeof(*search));
  lsa_place_params_init(&search->descriptor);
  search->min_travelled = 20.;
  search->exclusion_half_window = 5;
}

int lsa_scan_descriptor_host(const lsa_place_params_t* params, const lsa_point_t* pts, int n, float* out)
{
  if (!params) return LSA_E_ARG;
  return lsa::host::ScanDescriptor(*params, pts, n, out);
}

int lsa_place_distance_host(const lsa_place_params_t* params, const float* a, const float* b, float* distance, int* shift)
{
  if (!params) return LSA_E_ARG;
  return lsa::host::PlaceDistance(*params, a, b, distance, shift);
}

int lsa_place_select_host(const float* distance, const int32_t* shift, const double* poses17, int n, int query, int sectors, double min_travelled,
                          double max_distance, double max_descriptor_distance, int exclusion_half_window, lsa_place_candidate_t* out, int capacity)
{
  return lsa::host::PlaceSelect(distance, shift, poses17, n, query, sectors, min_travelled, max_distance, max_descriptor_distance, exclusion_half_window, out,
                                capacity);
}

void lsa_loop_detect_init(lsa_loop_detect_t* detect)
{
  if (!detect) return;
  std::memset(detect, 0, sizeof(*detect));
  lsa_place_search_init(&detect->search);
  detect->last_query = -1;
  detect->query_stride = 1;
  detect->per_query = 1;
}

int lsa_place_detect_host(const lsa_loop_detect_t* detect, const float* descriptors, const double* poses17, int n, lsa_loop_candidate_t* out, int capacity)
{
  lsa_loop_detect_t d;
  lsa_loop_detect_init(&d);
  if (detect) d = *detect;
  return lsa::host::PlaceDetect(d, descriptors, poses17, n, out, capacity);
}

void lsa_map_place_search_init(lsa_map_place_search_t* search)
{
  if (!search) return;
  std::memset(search, 0, sizeof(*search));
  lsa_place_params_init(&search->descriptor);
  search->exclusion_radius = 5.;
}

int lsa_map_descriptor_host(const lsa_place_params_t* params, const lsa_point_t* pts, int n, const double viewpoint[3], float* out)
{
  if (!params) return LSA_E_ARG;
  return lsa::host::MapDescriptor(*params, pts, n, viewpoint, out);
}

int lsa_map_place_select_host(const float* distance, const int32_t* shift, const double* viewpoints, int V, int sectors, const lsa_map_place_search_t* search,
                              lsa_map_place_candidate_t* out, int capacity)
{
  lsa_map_place_search_t s;
  lsa_map_place_search_init(&s);
  if (search) s = *search;
  return lsa::host::MapPlaceSelect(distance, shift, viewpoints, V, sectors, s, out, capacity);
}

}  // extern "C"
