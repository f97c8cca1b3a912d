// Driver of tests/test_lm_step_reference.py: the host's trust-region loop (lidarslam_amd/csrc/host/lsa_lm_loop.cpp) compiled
// with its own main under -fsanitize=address,undefined.  Reads the scripts the test wrote -- n, then per script two_d,
// max_iter, min_matches, K as int32, then the start points, then the sums, as lsa_selftest_lm_host takes them -- into
// buffers of exactly the sizes the call is documented with, so that a read or write past an end is the sanitizer's to
// find; runs them, writes records, results and status behind each other, and prints "ok".
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../include/lidarslam_amd.h"

template <typename T> static bool ReadAll(std::FILE* f, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
template <typename T> static bool WriteAll(std::FILE* f, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char** argv)
{
  if (argc != 3) { std::printf("usage: %s scripts.bin out.bin\n", argv[0]); return 2; }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::printf("cannot read %s\n", argv[1]); return 2; }
  int32_t n = 0;
  if (std::fread(&n, sizeof(n), 1, in) != 1 || n <= 0 || n > 65536) { std::printf("bad script count\n"); return 2; }
  std::vector<int32_t> header(static_cast<size_t>(n) * 4);
  if (!ReadAll(in, header)) { std::printf("short header\n"); return 2; }
  size_t total = 0;
  for (int s = 0; s < n; ++s)
  {
    if (header[4 * s + 3] < 1 || header[4 * s + 3] > 4096) { std::printf("bad script length\n"); return 2; }
    total += static_cast<size_t>(header[4 * s + 3]);
  }
  std::vector<double> x0(static_cast<size_t>(n) * 6), sums(total * 29);
  if (!ReadAll(in, x0) || !ReadAll(in, sums)) { std::printf("short scripts\n"); return 2; }
  std::fclose(in);
  std::vector<double> records(total * 42, -1.), results(static_cast<size_t>(n) * 45, -1.);
  std::vector<int32_t> status(static_cast<size_t>(n) * 2, -1);
  static_assert(sizeof(int32_t) == sizeof(int), "the header is an array of int");
  const int rc = lsa_selftest_lm_host(n, header.data(), x0.data(), sums.data(), records.data(), results.data(), status.data());
  if (rc != LSA_OK) { std::printf("lsa_selftest_lm_host returned %d\n", rc); return 1; }
  // the refusals write nothing
  if (lsa_selftest_lm_host(0, header.data(), x0.data(), sums.data(), records.data(), results.data(), status.data()) != LSA_E_ARG ||
      lsa_selftest_lm_host(n, nullptr, x0.data(), sums.data(), records.data(), results.data(), status.data()) != LSA_E_ARG)
  {
    std::printf("a bad argument was not refused\n");
    return 1;
  }
  std::FILE* out = std::fopen(argv[2], "wb");
  if (!out || !WriteAll(out, records) || !WriteAll(out, results) || !WriteAll(out, status) || std::fclose(out) != 0) { std::printf("cannot write %s\n", argv[2]); return 2; }
  std::printf("ok %d scripts, %zu evaluations\n", n, total);
  return 0;
}
