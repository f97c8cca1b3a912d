// lsa_place_select.h -- the gates and the ranking of loop detection over the whole log, ONE source for the host statement
// (host/lsa_place.cpp: lsa_place_detect_host) and the device (lsa_place_detect.hip): DESIGN.md 3.13.  Which logged frame i
// may answer query q, and which of two that may is the better one, is decided by the text below on both sides -- the same
// double arithmetic (IEEE sqrt, nothing contracted: -ffp-contract=off), the same comparisons in the same sense (a NaN fails
// every gate), so the same table and the same poses give the same candidates wherever this is compiled.  The rules are
// lsa_place_select_host's (PlaceSelect, host/lsa_place.cpp), which tests hold this text to.
#pragma once
#include "lsa_scan_descriptor.h"

namespace lsa
{
namespace place
{
constexpr int kMaxPerQuery = 16;  // candidates a query: the device selection keeps the picked frames in registers

// what the selection knows of a logged frame: its position and the way from frame 0 to it
struct FramePosition
{
  double x, y, z, travelled;
};
LSA_HDP double metres(const FramePosition& a, const FramePosition& b)
{
  const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return __builtin_sqrt(dx * dx + dy * dy + dz * dz);
}
// frame i lies at least minTravelled back along the trajectory from q.  travelled does not decrease with the frame, the
// rounded difference does not increase: the frames that pass are a prefix of 0..q-1
LSA_HDP bool travelled_gate(const FramePosition& q, const FramePosition& i, double minTravelled) { return q.travelled - i.travelled >= minTravelled; }
// ... within maxDistance of q's position (maxDistance <= 0: no gate)
LSA_HDP bool position_gate(const FramePosition& q, const FramePosition& i, double maxDistance) { return !(maxDistance > 0.) || metres(i, q) <= maxDistance; }
// ... looks enough like it (maxDescriptorDistance <= 0: no gate); a NaN has no rank
LSA_HDP bool descriptor_gate(float distance, double maxDescriptorDistance)
{
  if (distance != distance) return false;
  return !(maxDescriptorDistance > 0.) || (double)distance <= maxDescriptorDistance;
}
// frame i is within halfWindow frames of one already picked
LSA_HDP bool excluded_by(int i, int picked, int halfWindow)
{
  const long long d = (long long)i - (long long)picked;
  return (d < 0 ? -d : d) <= (long long)halfWindow;
}
// (d2, i2) ranks before (d, i): the smaller distance, the lower frame on a tie -- a total order on entries without NaN
LSA_HDP bool ranks_before(float d2, int i2, float d, int i) { return d2 < d || (d2 == d && i2 < i); }

// the limits of the selection's parameters (lsa_place_search_t beyond its descriptor) and of a query set on a log of n frames
LSA_HDP bool search_ok(const lsa_place_search_t& s)
{
  return params_ok(s.descriptor) && s.min_travelled >= 0. && s.exclusion_half_window >= 0 && s.max_distance == s.max_distance &&
         s.max_descriptor_distance == s.max_descriptor_distance;
}
// first, first + stride, ... <= last (last < 0: n - 1); false: not a query set of this log.  *last_out the resolved last
LSA_HDP bool query_set_ok(int n, int first, int last, int stride, int* last_out)
{
  if (n < 1 || stride < 1) return false;
  if (last < 0) last = n - 1;
  if (first < 0 || first > last || last >= n) return false;
  *last_out = last;
  return true;
}
LSA_HDP int query_count(int first, int last, int stride) { return (last - first) / stride + 1; }
}  // namespace place
}  // namespace lsa
