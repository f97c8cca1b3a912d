// Driver of tests/test_host_place.py: the host statement of place recognition -- a frame's descriptor, the distance of two
// descriptors and the selection of candidates (lidarslam_amd/csrc/host/lsa_place.cpp over lsa_scan_descriptor.h) -- compiled
// with its own main under -fsanitize=address,undefined.  Runs the shapes of the tests and the degenerate inputs, checks the
// answers that can be stated in a line, and prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "lsa_place.h"

using lsa::host::PlaceDistance;
using lsa::host::PlaceSelect;
using lsa::host::ScanDescriptor;

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

static lsa_point_t Point(float x, float y, float z)
{
  lsa_point_t p;
  std::memset(&p, 0, sizeof(p));
  p.x = x; p.y = y; p.z = z;
  return p;
}

// exactly `length` floats, so that a write past the end is the sanitizer's to find
static std::vector<float> Describe(const lsa_place_params_t& p, const std::vector<lsa_point_t>& pts)
{
  std::vector<float> out(static_cast<size_t>(lsa::place::length(p)), -1.f);
  CHECK(ScanDescriptor(p, pts.empty() ? nullptr : pts.data(), static_cast<int>(pts.size()), out.data()) == LSA_OK);
  return out;
}

static bool AllZero(const std::vector<float>& d)
{
  for (float v : d)
    if (v != 0.f) return false;
  return true;
}

int main()
{
  std::mt19937 rng(20261019);
  std::uniform_real_distribution<float> xy(-90.f, 90.f), zz(-5.f, 8.f);
  const int shapes[4][2] = {{1, 1}, {3, 7}, {20, 60}, {32, 120}};
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (const auto& shape : shapes)
  {
    lsa_place_params_t p;
    lsa_place_params_init(&p);
    p.rings = shape[0];
    p.sectors = shape[1];
    p.min_common_sectors = 0;  // the default of the shape
    CHECK(lsa::place::params_ok(p));
    const size_t cells = static_cast<size_t>(lsa::place::cells(p));
    // n = 0, all points NaN, r == max_range exactly, r just inside, far outside, infinite
    CHECK(AllZero(Describe(p, {})));
    CHECK(AllZero(Describe(p, {Point(nan, 1, 1), Point(1, nan, 1), Point(1, 1, nan), Point(nan, nan, nan)})));
    CHECK(AllZero(Describe(p, {Point(80.f, 0, 1), Point(0, -80.f, 1), Point(-80.f, 0, 1), Point(1e30f, 1e30f, 1), Point(inf, 0, 1), Point(0, -inf, 1), Point(3e38f, 3e38f, 1)})));
    {
      const std::vector<float> d = Describe(p, {Point(std::nextafter(80.f, 0.f), 0, 1)});  // the outermost ring, the sector of angle 0
      CHECK(d[(static_cast<size_t>(p.rings) - 1) * p.sectors + p.sectors / 2] == 3.f);
      const std::vector<float> e = Describe(p, {Point(-79.f, -0.f, 1), Point(-79.f, 0.f, 2)});  // angle pi: the last sector, not one past it
      CHECK(e[(static_cast<size_t>(p.rings) - 1) * p.sectors + p.sectors - 1] == 4.f);
      const std::vector<float> f = Describe(p, {Point(0, 0, 1), Point(-0.f, -0.f, 0.5f)});
      CHECK(f[p.sectors / 2] == 3.f);
    }
    // random clouds: every cell is a height seen, every norm the root of its column's squares; distances in [0, 2]
    std::vector<std::vector<float>> desc;
    for (int c = 0; c < 6; ++c)
    {
      std::vector<lsa_point_t> pts;
      const int n = c == 0 ? 0 : 50 * c * c;
      for (int i = 0; i < n; ++i) pts.push_back(Point(xy(rng), xy(rng), i % 17 == 0 ? nan : zz(rng)));
      desc.push_back(Describe(p, pts));
      for (int j = 0; j < p.sectors; ++j)
      {
        float sum = 0.f;
        for (int r = 0; r < p.rings; ++r)
        {
          const float v = desc.back()[static_cast<size_t>(r) * p.sectors + j];
          CHECK(v >= 0.f && v <= 10.f);
          sum += v * v;
        }
        CHECK(desc.back()[cells + j] == std::sqrt(sum));
      }
    }
    std::vector<float> distance;
    std::vector<int32_t> shift;
    for (size_t c = 0; c < desc.size(); ++c)
    {
      float d = -1.f;
      int s = -1;
      CHECK(PlaceDistance(p, desc[5].data(), desc[c].data(), &d, &s) == LSA_OK);
      CHECK(d >= -1e-5f && d <= 2.f && s >= 0 && s < p.sectors);
      if (c == 0) CHECK(d == 1.f && s == 0);
      if (c == 5) CHECK(std::fabs(d) <= 1e-5f && s == 0);
      distance.push_back(d);
      shift.push_back(s);
    }
    // the selection on a trajectory of as many poses, at every capacity, window and gate
    const int n = static_cast<int>(desc.size());
    std::vector<double> rows(static_cast<size_t>(n) * 17, 0.);
    for (int i = 0; i < n; ++i)
    {
      double* m = &rows[17 * static_cast<size_t>(i)];
      m[0] = m[5] = m[10] = m[15] = 1.;
      m[3] = 3. * i;
      m[16] = 0.1 * i;
    }
    for (int query = 0; query < n; ++query)
      for (int capacity = 0; capacity <= n; ++capacity)
        for (int window = 0; window <= n; window += 2)
          for (double gate : {0., 0.5, 2.})
          {
            std::vector<lsa_place_candidate_t> out(static_cast<size_t>(capacity));  // exactly `capacity`
            const int found = PlaceSelect(distance.data(), shift.data(), rows.data(), n, query, p.sectors, 3., gate * 6., gate, window, out.data(), capacity);
            CHECK(found >= 0 && found <= capacity && found <= query);
            for (int k = 0; k < found; ++k)
            {
              CHECK(out[k].frame >= 0 && out[k].frame < query && out[k].shift == shift[out[k].frame] && out[k].distance == distance[out[k].frame]);
              CHECK(out[k].yaw > -3.1415926535897936 && out[k].yaw <= 3.1415926535897936);
              if (k > 0) CHECK(out[k - 1].distance <= out[k].distance && std::abs(out[k].frame - out[k - 1].frame) > window);
            }
          }
    CHECK(PlaceSelect(nullptr, nullptr, rows.data(), n, 0, p.sectors, 0., 0., 0., 0, nullptr, 0) == 0);
    CHECK(PlaceSelect(distance.data(), shift.data(), rows.data(), n, n, p.sectors, 0., 0., 0., 0, nullptr, 0) == LSA_E_ARG);
    CHECK(PlaceSelect(distance.data(), shift.data(), nullptr, n, 1, p.sectors, 0., 0., 0., 0, nullptr, 0) == LSA_E_ARG);
  }
  // refusals write nothing
  {
    lsa_place_params_t p;
    lsa_place_params_init(&p);
    float one = 7.f;
    const lsa_point_t pt = Point(1, 1, 1);
    for (int bad = 0; bad < 7; ++bad)
    {
      lsa_place_params_t q = p;
      if (bad == 0) q.rings = 0;
      if (bad == 1) q.rings = 33;
      if (bad == 2) q.sectors = 121;
      if (bad == 3) q.type_mask = 0;
      if (bad == 4) q.max_range = q.min_range;
      if (bad == 5) q.height_offset = std::numeric_limits<double>::infinity();
      if (bad == 6) q.max_range = std::numeric_limits<double>::quiet_NaN();
      CHECK(ScanDescriptor(q, &pt, 1, &one) == LSA_E_ARG && one == 7.f);
      int s = 5;
      CHECK(PlaceDistance(q, &one, &one, &one, &s) == LSA_E_ARG && one == 7.f && s == 5);
    }
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
