// lsa_occupancy.cpp -- the writer of lsa_occupancy.h and its C export; no device code, no state but the error of the thread.
#include "lsa_occupancy.h"
#include <cstdio>
#include <vector>

namespace lsa
{
namespace occupancy
{
namespace
{
bool spill(const std::string& path, const void* head, size_t head_bytes, const void* body, size_t body_bytes, std::string& err)
{
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f)
  {
    err = path + ": cannot be opened for writing";
    return false;
  }
  bool ok = std::fwrite(head, 1, head_bytes, f) == head_bytes;
  ok = ok && (body_bytes == 0 || std::fwrite(body, 1, body_bytes, f) == body_bytes);
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) err = path + ": short write";
  return ok;
}
}  // namespace

long long write(const std::string& prefix, const lsa_dense_grid_info_t& info, const int8_t* state, std::string& err)
{
  if (info.width < 0 || info.height < 0)
  {
    err = prefix + ": a grid of negative size";
    return LSA_E_ARG;
  }
  const size_t w = static_cast<size_t>(info.width), h = static_cast<size_t>(info.height);
  if (w * h == 0) return 0;
  if (!state)
  {
    err = prefix + ": no states";
    return LSA_E_ARG;
  }
  // map_server's origin is the lower-left pixel: the image's first row is the grid's last
  std::vector<unsigned char> pixels(w * h);
  for (size_t row = 0; row < h; ++row)
  {
    const int8_t* from = state + (h - 1 - row) * w;
    unsigned char* to = pixels.data() + row * w;
    for (size_t x = 0; x < w; ++x) to[x] = grey_of(from[x]);
  }
  char head[64];
  const int head_bytes = std::snprintf(head, sizeof(head), "P5\n%d %d\n255\n", info.width, info.height);
  if (!spill(prefix + ".pgm", head, static_cast<size_t>(head_bytes), pixels.data(), pixels.size(), err)) return LSA_E_ARG;
  const size_t slash = prefix.find_last_of('/');
  const std::string name = (slash == std::string::npos ? prefix : prefix.substr(slash + 1)) + ".pgm";
  char numbers[128];
  std::snprintf(numbers, sizeof(numbers), "resolution: %.17g\norigin: [%.17g, %.17g, 0]\n", info.resolution, info.origin_x, info.origin_y);
  const std::string yaml = "image: " + name + "\n" + numbers + "negate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n";
  if (!spill(prefix + ".yaml", yaml.data(), yaml.size(), nullptr, 0, err)) return LSA_E_ARG;
  return static_cast<long long>(w * h);
}
}  // namespace occupancy
}  // namespace lsa

namespace
{
std::string& occupancy_error()
{
  thread_local std::string e;
  return e;
}
}  // namespace

extern "C" {

const char* lsa_occupancy_last_error(void) { return occupancy_error().c_str(); }

int lsa_occupancy_write(const char* prefix, const lsa_dense_grid_info_t* info, const int8_t* state)
{
  if (!prefix || !info)
  {
    occupancy_error() = "lsa_occupancy_write: bad argument";
    return LSA_E_ARG;
  }
  const long long n = lsa::occupancy::write(prefix, *info, state, occupancy_error());
  return n < 0 ? static_cast<int>(n) : LSA_OK;
}

}  // extern "C"
