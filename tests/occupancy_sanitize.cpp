// Driver of tests/test_dense_grid_host.py: the occupancy-grid writer (lidarslam_amd/csrc/host/lsa_occupancy.cpp) compiled with
// its own main under -fsanitize=address,undefined.  In the directory given it writes grids of 1 x 1, 3 x 2 (asymmetric, every
// state and a few values that are none of the three) and 257 x 129 cells from buffers of exactly width * height bytes, reads
// the files back and compares header, row flip and grey levels; then the refusals: no states, a negative size, a directory
// that does not exist; and a grid without cells, which writes nothing.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../lidarslam_amd/csrc/host/lsa_occupancy.h"

static bool Slurp(const std::string& path, std::vector<unsigned char>& out)
{
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  out.resize(static_cast<size_t>(std::ftell(f)));
  std::fseek(f, 0, SEEK_SET);
  const bool ok = out.empty() || std::fread(out.data(), 1, out.size(), f) == out.size();
  std::fclose(f);
  return ok;
}

static int Check(const std::string& dir, int w, int h)
{
  lsa_dense_grid_info_t info;
  std::memset(&info, 0, sizeof(info));
  info.cx0 = -7;
  info.cy0 = 3;
  info.width = w;
  info.height = h;
  info.resolution = 0.4;
  info.origin_x = -7 * 0.4;
  info.origin_y = 3 * 0.4;
  const int8_t values[6] = {100, 0, -1, 50, -128, 127};
  std::vector<int8_t> state(static_cast<size_t>(w) * h);  // exactly as many as the grid has cells
  for (size_t i = 0; i < state.size(); ++i) state[i] = values[(i * 7 + i / 5) % 6];
  const std::string prefix = dir + "/grid" + std::to_string(w);
  if (lsa_occupancy_write(prefix.c_str(), &info, state.data()) != LSA_OK) return 1;
  std::vector<unsigned char> pgm, yaml;
  if (!Slurp(prefix + ".pgm", pgm) || !Slurp(prefix + ".yaml", yaml)) return 2;
  const std::string head = "P5\n" + std::to_string(w) + " " + std::to_string(h) + "\n255\n";
  if (pgm.size() != head.size() + state.size() || std::memcmp(pgm.data(), head.data(), head.size()) != 0) return 3;
  for (int row = 0; row < h; ++row)
    for (int x = 0; x < w; ++x)
    {
      const int8_t s = state[static_cast<size_t>(h - 1 - row) * w + x];  // image row 0 is the grid's last row
      const unsigned char want = s == 100 ? 0 : (s == 0 ? 254 : 205);
      if (pgm[head.size() + static_cast<size_t>(row) * w + x] != want) return 4;
    }
  char want[256];
  std::snprintf(want, sizeof(want), "image: grid%d.pgm\nresolution: %.17g\norigin: [%.17g, %.17g, 0]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n", w,
                info.resolution, info.origin_x, info.origin_y);
  if (std::string(yaml.begin(), yaml.end()) != want) return 5;
  return 0;
}

int main(int argc, char** argv)
{
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const int sizes[3][2] = {{1, 1}, {3, 2}, {257, 129}};
  for (const auto& s : sizes)
    if (const int rc = Check(dir, s[0], s[1]))
    {
      std::printf("grid %d x %d: %d (%s)\n", s[0], s[1], rc, lsa_occupancy_last_error());
      return 1;
    }
  lsa_dense_grid_info_t info;
  std::memset(&info, 0, sizeof(info));
  const int8_t one = 0;
  // a grid without cells writes nothing and is no error
  if (lsa_occupancy_write((dir + "/none").c_str(), &info, nullptr) != LSA_OK || std::fopen((dir + "/none.pgm").c_str(), "rb")) return 1;
  info.width = info.height = 1;
  if (lsa_occupancy_write((dir + "/nostate").c_str(), &info, nullptr) != LSA_E_ARG) return 1;
  if (lsa_occupancy_write((dir + "/missing/grid").c_str(), &info, &one) != LSA_E_ARG || std::string(lsa_occupancy_last_error()).find("missing") == std::string::npos) return 1;
  if (lsa_occupancy_write(nullptr, &info, &one) != LSA_E_ARG || lsa_occupancy_write((dir + "/x").c_str(), nullptr, &one) != LSA_E_ARG) return 1;
  info.width = -1;
  if (lsa_occupancy_write((dir + "/negative").c_str(), &info, &one) != LSA_E_ARG) return 1;
  std::printf("ok\n");
  return 0;
}
