// lsa_pcd.h -- PCD v0.7 files of LidarPoint clouds (the keypoint maps Slam::SaveMapsToPCD / LoadMapsFromPCD exchange,
// slam_lib/src/Slam.cxx:504-543, slam_lib/include/LidarSlam/PointCloudStorage.h:60-115), written from the format's
// description, no PCL: header parser, ascii / binary / binary_compressed data sections, the LZF stream of the latter.
//
// A file's data section is one of two shapes: records (ascii rows are parsed into the records their header declares;
// binary files hold them) or, binary_compressed, one column per field, field after field.  Either way a LidarPoint field
// is found at base + i * step: the ColumnTable below says so for the eight fields a LidarPoint has, and decode_point turns
// point i into the 32-byte lsa_point_t -- on the host here, on the device in lsa_pcd.hip (k_pcd_decode), same function.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "../../../include/lidarslam_amd.h"

#if defined(__HIPCC__)
#define LSA_PCD_HD __host__ __device__
#else
#define LSA_PCD_HD
#endif

namespace lsa
{
namespace pcd
{

// the registered fields of LidarPoint in order (slam_lib/include/LidarSlam/LidarPoint.h:68-77): what a written file holds
enum { kX = 0, kY, kZ, kTime, kIntensity, kLaserId, kDeviceId, kLabel, kNbFields };
constexpr int kRecordBytes = 28;  // 4 4 4 8 4 2 1 1, packed
constexpr int kMaxFields = 16;    // columns a table can name (the eight of a LidarPoint, the four of a normal)
// the fields a dense map's normals add behind a LidarPoint's (pcl::Normal's names): four floats, 16 bytes
enum { kNormalX = kNbFields, kNormalY, kNormalZ, kCurvature, kNbColumns };
constexpr int kNormalBytes = 16;
enum { kAbsent = 0, kFloat = 1, kSigned = 2, kUnsigned = 3 };

struct Column
{
  int64_t base;   // byte offset of point 0's value in the data handed to decode_point
  int32_t step;   // bytes from one point's value to the next (records: the record size; columns: the value size)
  uint8_t size;   // 1, 2, 4, 8
  uint8_t type;   // kAbsent: the field is not in the file, its value is 0
  uint16_t pad;
};
struct ColumnTable
{
  Column c[kMaxFields];
};

// values are assembled from bytes: a record's fields sit at any offset
LSA_PCD_HD inline uint64_t load_bytes(const unsigned char* p, int size)
{
  uint64_t v = 0;
  for (int b = 0; b < size; ++b) v |= (uint64_t)p[b] << (8 * b);
  return v;
}

// the value of one field converted to T as C++ converts the file's type to T
template <typename T>
LSA_PCD_HD inline T convert_field(uint64_t bits, int size, int type)
{
  if (type == kFloat)
  {
    if (size == 8)
    {
      double d;
      memcpy(&d, &bits, 8);
      return static_cast<T>(d);
    }
    const uint32_t lo = (uint32_t)bits;
    float f;
    memcpy(&f, &lo, 4);
    return static_cast<T>(f);
  }
  if (type == kSigned)
  {
    const int sh = 64 - 8 * size;
    const int64_t s = (int64_t)(bits << sh) >> sh;
    return static_cast<T>(s);
  }
  return static_cast<T>(bits);
}

template <typename T>
LSA_PCD_HD inline T field_of(const unsigned char* data, const Column& c, long long i)
{
  if (c.type == kAbsent) return T(0);
  return convert_field<T>(load_bytes(data + c.base + i * c.step, c.size), c.size, c.type);
}

LSA_PCD_HD inline lsa_point_t decode_point(const unsigned char* data, const ColumnTable& t, long long i)
{
  lsa_point_t p;
  p.x = field_of<float>(data, t.c[kX], i);
  p.y = field_of<float>(data, t.c[kY], i);
  p.z = field_of<float>(data, t.c[kZ], i);
  p.w = 1.f;  // PCL_ADD_POINT4D: what a point loaded by PCL holds
  p.time = field_of<double>(data, t.c[kTime], i);
  p.intensity = field_of<float>(data, t.c[kIntensity], i);
  p.laser_id = field_of<uint16_t>(data, t.c[kLaserId], i);
  p.device_id = field_of<uint8_t>(data, t.c[kDeviceId], i);
  p.label = field_of<uint8_t>(data, t.c[kLabel], i);
  return p;
}

// the 28 bytes of a written record as seven 32-bit words
LSA_PCD_HD inline void encode_record(const lsa_point_t& p, uint32_t w[7])
{
  uint64_t t;
  memcpy(&w[0], &p.x, 4);
  memcpy(&w[1], &p.y, 4);
  memcpy(&w[2], &p.z, 4);
  memcpy(&t, &p.time, 8);
  w[3] = (uint32_t)t;
  w[4] = (uint32_t)(t >> 32);
  memcpy(&w[5], &p.intensity, 4);
  w[6] = (uint32_t)p.laser_id | ((uint32_t)p.device_id << 16) | ((uint32_t)p.label << 24);
}

enum Format { kAscii = 0, kBinary = 1, kBinaryCompressed = 2 };  // PCDFormat (PointCloudStorage.h:60-65)

struct Field
{
  std::string name;
  int offset = 0;  // byte offset in a record
  int size = 0;
  char type = 'F';
  int count = 1;
};

struct Header
{
  std::vector<Field> fields;
  long long width = 0, height = 1, points = 0;
  int format = kAscii;
  long long data_offset = 0;  // first byte of the data section
  int record_bytes = 0;       // sum of size * count
  int data_line = 0;          // line of the DATA entry
};

// A file's data section in memory, ready for decode_point.  `columns`: one column per field (binary_compressed),
// else records of header.record_bytes.
struct Cloud
{
  Header header;
  bool columns = false;
  std::vector<unsigned char> data;
  ColumnTable table;
};

// seconds spent by the last read_* / write of this thread: [0] file, [1] LZF, [2] ascii conversion
struct Timing
{
  double file = 0, lzf = 0, text = 0;
};
Timing& timing();

// All return LSA_OK or LSA_E_ARG with `err` naming the file (and the header line where there is one).
int read_header(const std::string& path, Header& h, std::string& err);
// the table of a header's fields for records (columns = false) or for the columns of n points
ColumnTable table_of(const Header& h, bool columns, long long n);
// header + data section: ascii rows parsed into records, binary records as they are, binary_compressed decompressed
// into its columns.  With raw_binary = false the records of a binary file are not read (data stays empty): the caller
// streams them from header.data_offset itself.
int read_cloud(const std::string& path, Cloud& c, std::string& err, bool raw_binary = true);
int read_points(const std::string& path, std::vector<lsa_point_t>& out, std::string& err);
// Writes the LidarPoint field list.  `records`: n packed 28-byte records; `columns` (binary_compressed only, may be
// null: made from the records): the eight columns of n points, field after field.  n == 0 writes nothing and returns -3,
// savePointCloudToPCD's result for an empty cloud (PointCloudStorage.h:91-92); an unknown format returns -4 (:111-113).
// `normals4` (may be null: the file is the LidarPoint's alone, as ever): n x 4 floats normal_x normal_y normal_z curvature,
// written as four more fields behind the eight, 44 bytes a record.
int write_records(const std::string& path, const unsigned char* records, const unsigned char* columns, long long n, int format, std::string& err,
                  const float* normals4 = nullptr);
// the four floats per point of a file that has the fields normal_x normal_y normal_z curvature, each a 4-byte F of COUNT 1
int read_normals(const std::string& path, std::vector<float>& out4, std::string& err);
int write_points(const std::string& path, const lsa_point_t* pts, long long n, int format, std::string& err);

// LZF: a stream of literal runs (control byte c < 32: c + 1 bytes follow) and back references (c >> 5 = length - 2, 7
// meaning one more byte of length follows; then the low byte of the distance - 1, whose high five bits are c & 31).
std::vector<unsigned char> lzf_compress(const unsigned char* in, size_t n);
// returns the number of bytes written, or -1 when the stream is malformed or does not fit `capacity`
long long lzf_decompress(const unsigned char* in, size_t n, unsigned char* out, size_t capacity);

// Utils::Plural(KeypointTypeNames.at(k)) + ".pcd" (Slam.cxx:512, 530): edges / planes / blobs
const char* map_file_suffix(int type);

}  // namespace pcd
}  // namespace lsa
