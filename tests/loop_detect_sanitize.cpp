// Driver of tests/test_loop_detect_host.py: the host statement of loop detection over a whole log (PlaceDetect,
// lidarslam_amd/csrc/host/lsa_place.cpp) and the gates and ranking the device shares with it (lsa_place_select.h), compiled
// with its own main under -fsanitize=address,undefined.  Every output buffer is exactly as long as the call may fill it;
// each answer is checked against PlaceSelect on the table of PlaceDistance, and against a selection written with the shared
// text alone -- what k_place_select_rows does, one lane at a time.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "lsa_place.h"

using lsa::host::PlaceDetect;
using lsa::host::PlaceDistance;
using lsa::host::PlaceSelect;
namespace place = lsa::place;

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

// the device's selection for one query, sequentially: the travelled gate as a prefix, then rounds of the arg-min
static int SelectBySharedText(const lsa_place_search_t& s, const float* distance, const int32_t* shift, const place::FramePosition* pos, int q, int perQuery,
                              lsa_loop_candidate_t* out)
{
  int len = 0;
  while (len < q && place::travelled_gate(pos[q], pos[len], s.min_travelled)) ++len;
  for (int i = len; i < q; ++i) CHECK(!place::travelled_gate(pos[q], pos[i], s.min_travelled));  // a prefix indeed
  int picked[place::kMaxPerQuery];
  int found = 0;
  while (found < perQuery)
  {
    int best = -1;
    for (int i = len - 1; i >= 0; --i)  // (descending: the order of the scan must not matter)
    {
      if (!place::descriptor_gate(distance[i], s.max_descriptor_distance) || !place::position_gate(pos[q], pos[i], s.max_distance)) continue;
      bool excluded = false;
      for (int k = 0; k < found; ++k) excluded = excluded || place::excluded_by(i, picked[k], s.exclusion_half_window);
      if (excluded) continue;
      if (best < 0 || place::ranks_before(distance[i], i, distance[best], best)) best = i;
    }
    if (best < 0) break;
    picked[found] = best;
    lsa_loop_candidate_t c;
    std::memset(&c, 0, sizeof(c));
    c.query = q;
    c.frame = best;
    c.shift = shift[best];
    c.distance = distance[best];
    c.yaw = place::yaw_of(shift[best], s.descriptor.sectors);
    out[found++] = c;
  }
  return found;
}

int main()
{
  std::mt19937 rng(20261020);
  std::uniform_real_distribution<float> cell(0.f, 4.f), coin(0.f, 1.f);
  const int shapes[3][2] = {{1, 1}, {3, 7}, {20, 60}};
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (const auto& shape : shapes)
    for (int n : {1, 2, 3, 24})
    {
      lsa_loop_detect_t d;
      lsa_loop_detect_init(&d);
      d.search.descriptor.rings = shape[0];
      d.search.descriptor.sectors = shape[1];
      d.search.descriptor.min_common_sectors = 0;
      const lsa_place_params_t& p = d.search.descriptor;
      const size_t length = static_cast<size_t>(place::length(p)), cells = static_cast<size_t>(place::cells(p));
      // descriptors: random, every fourth identical to frame 0, every fifth empty, one with a NaN cell
      std::vector<float> D(static_cast<size_t>(n) * length, 0.f);
      for (int i = 0; i < n; ++i)
      {
        float* f = &D[static_cast<size_t>(i) * length];
        if (i % 5 == 4) continue;
        if (i % 4 == 0 && i > 0) { std::memcpy(f, &D[0], length * sizeof(float)); continue; }
        for (size_t c = 0; c < cells; ++c) f[c] = coin(rng) < 0.8f ? cell(rng) : 0.f;
        if (i == 7) f[0] = nan;
        for (int j = 0; j < p.sectors; ++j) f[cells + j] = place::column_norm(f, p.rings, p.sectors, j);
      }
      // out and back with a stationary stretch
      std::vector<double> rows(static_cast<size_t>(n) * 17, 0.);
      for (int i = 0; i < n; ++i)
      {
        double* m = &rows[17 * static_cast<size_t>(i)];
        m[0] = m[5] = m[10] = m[15] = 1.;
        m[3] = i < n / 2 ? 1. * i : (i < n / 2 + 3 ? 1. * (n / 2 - 1) : 1. * (n - 1 - i));
        m[7] = i < n / 2 ? 0. : 0.25;
        m[16] = 0.1 * i;
      }
      std::vector<place::FramePosition> pos(static_cast<size_t>(n));
      lsa::host::FramePositions(rows.data(), n, pos.data());
      for (int i = 1; i < n; ++i) CHECK(pos[i].travelled >= pos[i - 1].travelled);
      // the table, once
      std::vector<std::vector<float>> distance(static_cast<size_t>(n));
      std::vector<std::vector<int32_t>> shift(static_cast<size_t>(n));
      for (int q = 0; q < n; ++q)
        for (int i = 0; i < q; ++i)
        {
          float dd = -1.f;
          int ss = -1;
          CHECK(PlaceDistance(p, &D[static_cast<size_t>(q) * length], &D[static_cast<size_t>(i) * length], &dd, &ss) == LSA_OK);
          distance[q].push_back(dd);
          shift[q].push_back(ss);
        }
      for (int stride : {1, 3, n + 1})
        for (int perQuery : {1, 3, 16})
          for (int window : {0, 2, n})
            for (double travelled : {0., 3.})
              for (double gate : {0., 1.})
              {
                d.query_stride = stride;
                d.per_query = perQuery;
                d.first_query = 0;
                d.last_query = gate > 0. ? n - 1 : -1;
                d.search.min_travelled = travelled;
                d.search.max_distance = gate * 2.5;
                d.search.max_descriptor_distance = gate * 0.3;
                d.search.exclusion_half_window = window;
                const int queries = (n - 1) / stride + 1;
                std::vector<lsa_loop_candidate_t> out(static_cast<size_t>(queries) * perQuery);  // exactly what the call asks for
                const int found = PlaceDetect(d, D.data(), rows.data(), n, out.data(), static_cast<int>(out.size()));
                CHECK(found >= 0 && found <= static_cast<int>(out.size()));
                CHECK(PlaceDetect(d, D.data(), rows.data(), n, out.data(), static_cast<int>(out.size()) - 1) == LSA_E_ARG);
                int at = 0;
                for (int q = 0; q < n; q += stride)
                {
                  lsa_place_candidate_t want[place::kMaxPerQuery];
                  lsa_loop_candidate_t twin[place::kMaxPerQuery];
                  const int w = PlaceSelect(distance[q].data(), shift[q].data(), rows.data(), n, q, p.sectors, travelled, gate * 2.5, gate * 0.3, window, want, perQuery);
                  const int t = SelectBySharedText(d.search, distance[q].data(), shift[q].data(), pos.data(), q, perQuery, twin);
                  CHECK(w >= 0 && t == w && at + w <= found);
                  for (int k = 0; k < w && at + k < found; ++k)
                  {
                    const lsa_loop_candidate_t& c = out[static_cast<size_t>(at + k)];
                    CHECK(c.query == q && c.frame == want[k].frame && c.shift == want[k].shift && std::memcmp(&c.distance, &want[k].distance, 4) == 0 && c.yaw == want[k].yaw);
                    CHECK(std::memcmp(&c, &twin[k], sizeof(c)) == 0);
                    CHECK(c.frame != 7 || n <= 7 || c.distance == c.distance);
                  }
                  at += w;
                }
                CHECK(at == found);
              }
    }
  // refusals write nothing
  {
    lsa_loop_detect_t d;
    lsa_loop_detect_init(&d);
    d.search.descriptor.rings = 1;
    d.search.descriptor.sectors = 1;
    const float D[4] = {1.f, 1.f, 1.f, 1.f};
    double rows[34] = {0.};
    lsa_loop_candidate_t out[2];
    std::memset(out, 0x5A, sizeof(out));
    lsa_loop_candidate_t before[2];
    std::memcpy(before, out, sizeof(out));
    for (int bad = 0; bad < 8; ++bad)
    {
      lsa_loop_detect_t e = d;
      if (bad == 0) e.query_stride = 0;
      if (bad == 1) e.per_query = 0;
      if (bad == 2) e.per_query = 17;
      if (bad == 3) e.first_query = 2;
      if (bad == 4) e.last_query = 2;
      if (bad == 5) e.search.descriptor.sectors = 121;
      if (bad == 6) e.search.min_travelled = -1.;
      if (bad == 7) e.search.max_distance = std::numeric_limits<double>::quiet_NaN();
      CHECK(PlaceDetect(e, D, rows, 2, out, 2) == LSA_E_ARG && std::memcmp(before, out, sizeof(out)) == 0);
    }
    CHECK(PlaceDetect(d, D, rows, 2, out, 1) == LSA_E_ARG && std::memcmp(before, out, sizeof(out)) == 0);
    CHECK(PlaceDetect(d, D, rows, 0, out, 2) == LSA_E_ARG);
    d.query_stride = std::numeric_limits<int>::max();  // first + stride is never formed
    d.search.min_travelled = 0.;
    CHECK(PlaceDetect(d, D, rows, 2, out, 2) == 0);
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
