// Driver of tests/test_dense_normals_host.py: the PCD writer with the four normal fields and lsa_pcd_read_normals
// (lidarslam_amd/csrc/host/lsa_pcd.cpp) compiled with their own main under -fsanitize=address,undefined.  In the directory
// given it writes a cloud with normals -- rows of the "no normal" NaN among them -- in the three formats, reads points and
// normals back into buffers of exactly the sizes asked for and compares the bytes; then the refusals: a truncated data
// section per format, a header lacking one normal field, a normal field that is no 4-byte F, a file without normals.
// Prints "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../lidarslam_amd/csrc/host/lsa_pcd.h"

namespace pcd = lsa::pcd;

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

static bool Spill(const std::string& path, const unsigned char* data, size_t n)
{
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(data, 1, n, f) == n;
  return std::fclose(f) == 0 && ok;
}

static int Refused(const std::string& path, const char* what)
{
  std::vector<float> four(4);
  const int rc = lsa_pcd_read_normals(path.c_str(), four.data(), 1);
  if (rc != LSA_E_ARG || std::string(lsa_pcd_last_error()).find(path) == std::string::npos)
  {
    std::printf("%s: read_normals returned %d (%s)\n", what, rc, lsa_pcd_last_error());
    return 1;
  }
  return 0;
}

int main(int argc, char** argv)
{
  if (argc != 2) { std::printf("usage: %s directory\n", argv[0]); return 2; }
  const std::string dir = argv[1];
  const int n = 1003;
  std::vector<lsa_point_t> pts(n);
  std::vector<float> normals(static_cast<size_t>(n) * 4);
  const uint32_t nan_bits = 0x7fc00000u;
  for (int i = 0; i < n; ++i)
  {
    lsa_point_t& p = pts[i];
    p.x = 0.37f * i - 100.f; p.y = -1.0f / (i + 1); p.z = 1e-3f * i * i; p.w = 1.f;
    p.time = -0.1 + 1e-6 * i; p.intensity = static_cast<float>(i % 251);
    p.laser_id = static_cast<uint16_t>(i % 128); p.device_id = static_cast<uint8_t>(i % 2); p.label = static_cast<uint8_t>(i % 3);
    for (int k = 0; k < 4; ++k)
    {
      float v = std::sin(0.1f * i + k) * (k == 3 ? 0.3f : 1.f);
      if (i % 7 == 3) std::memcpy(&v, &nan_bits, 4);
      if (i % 11 == 5 && k < 3) v = k == 1 ? -0.f : 0.f;
      normals[static_cast<size_t>(i) * 4 + k] = v;
    }
  }
  std::vector<unsigned char> records(static_cast<size_t>(n) * pcd::kRecordBytes);
  for (int i = 0; i < n; ++i)
  {
    uint32_t w[7];
    pcd::encode_record(pts[i], w);
    std::memcpy(records.data() + static_cast<size_t>(i) * pcd::kRecordBytes, w, pcd::kRecordBytes);
  }
  static const char* const names[3] = {"ascii", "binary", "binary_compressed"};
  for (int format = 0; format < 3; ++format)
  {
    const std::string path = dir + "/normals_" + names[format] + ".pcd", plain = dir + "/plain_" + names[format] + ".pcd";
    std::string err;
    int rc = pcd::write_records(path, records.data(), nullptr, n, format, err, normals.data());
    if (rc != LSA_OK) { std::printf("%s: write returned %d (%s)\n", names[format], rc, err.c_str()); return 1; }
    rc = pcd::write_records(plain, records.data(), nullptr, n, format, err);
    if (rc != LSA_OK) { std::printf("%s: plain write returned %d (%s)\n", names[format], rc, err.c_str()); return 1; }
    // buffers of exactly n: a write past an end is the sanitizer's to find
    std::vector<lsa_point_t> back(n);
    std::vector<float> back4(static_cast<size_t>(n) * 4);
    if (lsa_pcd_read(path.c_str(), back.data(), n) != n || std::memcmp(back.data(), pts.data(), sizeof(lsa_point_t) * n) != 0)
    {
      std::printf("%s: the points do not read back (%s)\n", names[format], lsa_pcd_last_error());
      return 1;
    }
    if (lsa_pcd_read_normals(path.c_str(), back4.data(), n) != n || std::memcmp(back4.data(), normals.data(), sizeof(float) * 4 * n) != 0)
    {
      std::printf("%s: the normals do not read back (%s)\n", names[format], lsa_pcd_last_error());
      return 1;
    }
    // a smaller capacity: the count all the same, nothing past the capacity
    std::vector<float> few(4 * 5);
    if (lsa_pcd_read_normals(path.c_str(), few.data(), 5) != n || std::memcmp(few.data(), normals.data(), sizeof(float) * 20) != 0 ||
        lsa_pcd_read_normals(path.c_str(), nullptr, 0) != n)
    {
      std::printf("%s: the capacity rule\n", names[format]);
      return 1;
    }
    if (lsa_pcd_read(plain.c_str(), back.data(), n) != n || std::memcmp(back.data(), pts.data(), sizeof(lsa_point_t) * n) != 0)
    {
      std::printf("%s: the plain file does not read back\n", names[format]);
      return 1;
    }
    if (Refused(plain, "a file without normals")) return 1;
    // a truncated data section
    std::vector<unsigned char> bytes;
    if (!Slurp(path, bytes) || bytes.size() < 4000) { std::printf("cannot read %s back\n", path.c_str()); return 1; }
    const std::string cut = dir + "/cut_" + names[format] + ".pcd";
    if (!Spill(cut, bytes.data(), bytes.size() - bytes.size() / 3)) return 1;
    if (Refused(cut, "a truncated data section")) return 1;
    if (lsa_pcd_read(cut.c_str(), back.data(), n) != LSA_E_ARG) { std::printf("%s: a truncated file gave points\n", names[format]); return 1; }
  }
  // a header lacking one normal field, and one whose curvature is a double
  {
    const std::string lacking = dir + "/lacking.pcd", wide = dir + "/wide.pcd";
    const std::string a = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y curvature\nSIZE 4 4 4 4 4 4\nTYPE F F F F F F\n"
                          "COUNT 1 1 1 1 1 1\nWIDTH 2\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 2\nDATA ascii\n1 2 3 0 1 0\n4 5 6 nan nan nan\n";
    const std::string b = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z curvature\nSIZE 4 4 4 4 4 4 8\nTYPE F F F F F F F\n"
                          "COUNT 1 1 1 1 1 1 1\nWIDTH 2\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 2\nDATA ascii\n1 2 3 0 1 0 0.5\n4 5 6 nan nan nan nan\n";
    if (!Spill(lacking, reinterpret_cast<const unsigned char*>(a.data()), a.size()) || !Spill(wide, reinterpret_cast<const unsigned char*>(b.data()), b.size())) return 1;
    if (Refused(lacking, "a header lacking normal_z") || Refused(wide, "a curvature of 8 bytes")) return 1;
    std::vector<lsa_point_t> two(2);
    if (lsa_pcd_read(lacking.c_str(), two.data(), 2) != 2 || two[1].z != 6.f) { std::printf("the points of the lacking file\n"); return 1; }
  }
  std::printf("ok\n");
  return 0;
}
