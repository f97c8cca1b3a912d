// Driver of tests/test_host_loop_closure.py: the host-only parts of the loop-closure registration -- the candidate search on a
// trajectory and the windows of logged frames with their refusals (lidarslam_amd/csrc/host/lsa_loop_closure.h) -- compiled
// with their own main under -fsanitize=address,undefined.  Checks every answer against a statement written out here and
// prints "ok".
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>
#include "lsa_loop_closure.h"

using lsa::host::LoopClosureCandidate;
using lsa::host::LoopClosureWindows;
using lsa::host::LoopClosureWindowsOf;

static int failures = 0;
#define CHECK(cond)                                                       \
  do                                                                      \
  {                                                                       \
    if (!(cond))                                                          \
    {                                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static std::vector<double> Rows(const std::vector<std::array<double, 3>>& xyz)
{
  std::vector<double> rows(xyz.size() * 17, 0.);
  for (size_t i = 0; i < xyz.size(); ++i)
  {
    double* m = &rows[17 * i];
    m[0] = m[5] = m[10] = m[15] = 1.;
    m[3] = xyz[i][0]; m[7] = xyz[i][1]; m[11] = xyz[i][2];
    m[16] = 100. + 0.1 * i;
  }
  return rows;
}

static double Dist(const std::array<double, 3>& a, const std::array<double, 3>& b)
{
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return std::sqrt(dx * dx + dy * dy + dz * dz);
}

static int Brute(const std::vector<std::array<double, 3>>& xyz, int query, double minTravelled, double maxDistance)
{
  int best = -1;
  double bestD = 0.;
  for (int i = 0; i < query; ++i)
  {
    double way = 0.;  // from i to query, front to back like the helper's running sum
    std::vector<double> cum(query + 1, 0.);
    for (int j = 1; j <= query; ++j) cum[j] = cum[j - 1] + Dist(xyz[j], xyz[j - 1]);
    way = cum[query] - cum[i];
    if (!(way >= minTravelled)) continue;
    const double d = Dist(xyz[i], xyz[query]);
    if (!(d <= maxDistance)) continue;
    if (best < 0 || d < bestD) { best = i; bestD = d; }
  }
  return best;
}

int main()
{
  // ---- the candidate search
  {
    std::vector<std::array<double, 3>> line;
    for (int i = 0; i < 40; ++i) line.push_back({0.5 * i, 0., 0.});
    const std::vector<double> rows = Rows(line);
    CHECK(LoopClosureCandidate(rows.data(), 40, 39, 5., 2.) == -1);
    CHECK(LoopClosureCandidate(rows.data(), 40, 39, 0., 2.) == 38);
    CHECK(LoopClosureCandidate(rows.data(), 40, 0, 0., 1e9) == -1);  // nothing before the first frame
    CHECK(LoopClosureCandidate(rows.data(), 1, 0, 0., 1e9) == -1);
    CHECK(LoopClosureCandidate(nullptr, 40, 3, 1., 1.) == LSA_E_ARG);
    CHECK(LoopClosureCandidate(rows.data(), 0, 0, 1., 1.) == LSA_E_ARG);
    CHECK(LoopClosureCandidate(rows.data(), 40, -1, 1., 1.) == LSA_E_ARG);
    CHECK(LoopClosureCandidate(rows.data(), 40, 40, 1., 1.) == LSA_E_ARG);
    CHECK(LoopClosureCandidate(rows.data(), 40, 3, -1., 1.) == LSA_E_ARG);
    CHECK(LoopClosureCandidate(rows.data(), 40, 3, 1., std::numeric_limits<double>::quiet_NaN()) == LSA_E_ARG);
    CHECK(LoopClosureCandidate(rows.data(), 40, std::numeric_limits<int>::max(), 1., 1.) == LSA_E_ARG);
  }
  {
    std::mt19937_64 rng(7);
    std::normal_distribution<double> step(0., 1.);
    for (int trial = 0; trial < 20; ++trial)
    {
      const int n = 1 + (int)(rng() % 200);
      std::vector<std::array<double, 3>> walk(n);
      std::array<double, 3> at{0., 0., 0.};
      for (int i = 0; i < n; ++i)
      {
        at = {at[0] + step(rng), at[1] + step(rng), at[2] + 0.05 * step(rng)};
        walk[i] = at;
      }
      const std::vector<double> rows = Rows(walk);  // exactly n rows: a read past them is the sanitizer's to find
      for (int q : {0, n / 2, n - 1})
        for (double mt : {0., 10., 1e9})
          for (double md : {0., 2., 1e9}) CHECK(LoopClosureCandidate(rows.data(), n, q, mt, md) == Brute(walk, q, mt, md));
    }
  }
  // ---- the windows and their refusals
  {
    LoopClosureWindows w;
    std::string why;
    CHECK(LoopClosureWindowsOf(12, 9, 3, 2, 0, &w, &why) == LSA_OK && w.r0 == 1 && w.r1 == 5 && w.q0 == 9 && w.q1 == 9);
    CHECK(LoopClosureWindowsOf(12, 9, 1, 2, 0, &w, &why) == LSA_OK && w.r0 == 0 && w.r1 == 3);        // clipped at frame 0
    CHECK(LoopClosureWindowsOf(12, 11, 2, 1, 3, &w, &why) == LSA_OK && w.q0 == 8 && w.q1 == 11);      // clipped at the end
    CHECK(LoopClosureWindowsOf(12, 3, 9, 2, 0, &w, &why) == LSA_OK && w.r0 == 7 && w.r1 == 11);       // a query before the revisited frames
    CHECK(LoopClosureWindowsOf(12, 6, 3, 2, 0, &w, &why) == LSA_OK && w.r1 == 5 && w.q0 == 6);        // neighbours do not overlap
    CHECK(LoopClosureWindowsOf(2, 1, 0, 0, 0, &w, &why) == LSA_OK);
    const LoopClosureWindows kept = w;
    auto refused = [&](int logged, int q, int r, int wr, int wq) {
      why.clear();
      const int rc = LoopClosureWindowsOf(logged, q, r, wr, wq, &w, &why);
      return rc == LSA_E_ARG && !why.empty() && w.r0 == kept.r0 && w.r1 == kept.r1 && w.q0 == kept.q0 && w.q1 == kept.q1;
    };
    CHECK(refused(12, 5, 3, 2, 0));    // overlap at frame 5
    CHECK(refused(12, 9, 3, 2, 4));    // overlap: 1..5 and 5..11
    CHECK(refused(12, 3, 3, 0, 0));    // the same frame
    CHECK(refused(12, 9, 3, 100, 0));  // a window as wide as the log
    CHECK(refused(12, 12, 3, 2, 0));
    CHECK(refused(12, -1, 3, 2, 0));
    CHECK(refused(12, 9, 12, 2, 0));
    CHECK(refused(12, 9, -1, 2, 0));
    CHECK(refused(12, 9, 3, -1, 0));
    CHECK(refused(12, 9, 3, 2, -1));
    CHECK(refused(0, 0, 0, 0, 0));
    CHECK(refused(1, 0, 0, 0, 0));
    const int big = std::numeric_limits<int>::max();
    CHECK(refused(12, 9, 3, big, 0));  // no overflow on the way to the refusal
    CHECK(refused(big, big - 1, 0, 5, big));  // the query window reaches back over the whole log
    CHECK(LoopClosureWindowsOf(big, big - 1, 0, 5, 3, &w, &why) == LSA_OK && w.r0 == 0 && w.r1 == 5 && w.q0 == big - 4 && w.q1 == big - 1);
    w = kept;
    CHECK(LoopClosureWindowsOf(12, 9, 3, 2, 0, nullptr, &why) == LSA_E_ARG);
    CHECK(LoopClosureWindowsOf(12, 9, 3, 2, 0, &w, nullptr) == LSA_OK);
    CHECK(LoopClosureWindowsOf(12, 5, 3, 2, 0, &w, nullptr) == LSA_E_ARG);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
