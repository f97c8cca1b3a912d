// lsa_loop_closure.h -- the host-only parts of the registration of logged frames (SlamCore::RegisterLoggedFrames): the two
// windows of logged frames with their refusals, and the candidate search on a trajectory.  No device, no state: plain
// functions, so that a stand-alone program can run them under the sanitizers (tests/loop_closure_sanitize.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>
#include "../../../include/lidarslam_amd.h"

namespace lsa
{
namespace host
{

struct LoopClosureWindows
{
  int r0 = 0, r1 = 0;  // the revisited frames, inclusive: the target
  int q0 = 0, q1 = 0;  // the query frames, inclusive
};

// R = [revisited - wr, revisited + wr] and Q = [query - wq, query + wq], clipped to the `logged` frames.  LSA_E_ARG (and
// `why`) for an index outside the log, a negative half window, or windows that share a frame.
inline int LoopClosureWindowsOf(int logged, int query, int revisited, int wr, int wq, LoopClosureWindows* out, std::string* why)
{
  auto refuse = [&](const std::string& what) {
    if (why) *why = what;
    return LSA_E_ARG;
  };
  if (!out) return refuse("no place for the windows");
  if (logged < 1) return refuse("no logged frame");
  if (query < 0 || query >= logged) return refuse("query frame " + std::to_string(query) + " is not one of the " + std::to_string(logged) + " logged ones");
  if (revisited < 0 || revisited >= logged) return refuse("revisited frame " + std::to_string(revisited) + " is not one of the " + std::to_string(logged) + " logged ones");
  if (wr < 0 || wq < 0) return refuse("a half window is negative");
  const long long last = logged - 1;
  LoopClosureWindows w;
  w.r0 = static_cast<int>(std::max<long long>(0, static_cast<long long>(revisited) - wr));
  w.r1 = static_cast<int>(std::min<long long>(last, static_cast<long long>(revisited) + wr));
  w.q0 = static_cast<int>(std::max<long long>(0, static_cast<long long>(query) - wq));
  w.q1 = static_cast<int>(std::min<long long>(last, static_cast<long long>(query) + wq));
  if (w.r0 <= w.q1 && w.q0 <= w.r1)
    return refuse("the revisited frames " + std::to_string(w.r0) + ".." + std::to_string(w.r1) + " and the query frames " + std::to_string(w.q0) + ".." + std::to_string(w.q1) + " overlap");
  *out = w;
  return LSA_OK;
}

// lsa_loop_closure_candidate: rows of 17 doubles (row-major 4x4 + time).  Among the frames i < query whose way to query
// along the trajectory (the sum of the step lengths) is at least minTravelled and whose position is at most maxDistance
// from query's, the nearest; the lower index on a tie.  -1: none.
inline int LoopClosureCandidate(const double* poses17, int n, int query, double minTravelled, double maxDistance)
{
  if (!poses17 || n < 1 || query < 0 || query >= n || !(minTravelled >= 0.) || !(maxDistance >= 0.)) return LSA_E_ARG;
  auto position = [&](int i, int d) { return poses17[17 * static_cast<size_t>(i) + 4 * d + 3]; };
  auto distance = [&](int a, int b) {
    const double dx = position(a, 0) - position(b, 0), dy = position(a, 1) - position(b, 1), dz = position(a, 2) - position(b, 2);
    return std::sqrt(dx * dx + dy * dy + dz * dz);
  };
  // travelled[i]: the way from frame 0 to frame i
  std::vector<double> travelled(static_cast<size_t>(query) + 1, 0.);
  for (int i = 1; i <= query; ++i) travelled[i] = travelled[i - 1] + distance(i, i - 1);
  int best = -1;
  double bestDistance = 0.;
  for (int i = 0; i < query; ++i)
  {
    if (!(travelled[query] - travelled[i] >= minTravelled)) continue;
    const double d = distance(i, query);
    if (!(d <= maxDistance)) continue;
    if (best < 0 || d < bestDistance) { best = i; bestDistance = d; }
  }
  return best;
}

}  // namespace host
}  // namespace lsa
