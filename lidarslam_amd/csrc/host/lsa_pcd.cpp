// lsa_pcd.cpp -- host PCD codec (see lsa_pcd.h) and its C exports lsa_pcd_info / lsa_pcd_read / lsa_pcd_write.
#include "lsa_pcd.h"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <sstream>

namespace lsa
{
namespace pcd
{
namespace
{
double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

const char* const kFieldNames[kNbColumns] = {"x", "y", "z", "time", "intensity", "laser_id", "device_id", "label", "normal_x", "normal_y", "normal_z", "curvature"};
const int kFieldSizes[kNbColumns] = {4, 4, 4, 8, 4, 2, 1, 1, 4, 4, 4, 4};
const char kFieldTypes[kNbColumns] = {'F', 'F', 'F', 'F', 'F', 'U', 'U', 'U', 'F', 'F', 'F', 'F'};

struct File
{
  FILE* f = nullptr;
  ~File() { if (f) std::fclose(f); }
};

int bad(std::string& err, const std::string& path, int line, const std::string& what)
{
  err = path + (line > 0 ? ":" + std::to_string(line) : std::string()) + ": " + what;
  return LSA_E_ARG;
}

bool parse_int(const std::string& s, long long& v)
{
  if (s.empty()) return false;
  char* end = nullptr;
  v = std::strtoll(s.c_str(), &end, 10);
  return end && *end == 0;
}
}  // namespace

Timing& timing()
{
  thread_local Timing t;
  return t;
}

const char* map_file_suffix(int type) { return type == LSA_EDGE ? "edges.pcd" : type == LSA_PLANE ? "planes.pcd" : "blobs.pcd"; }

int read_header(const std::string& path, Header& h, std::string& err)
{
  h = Header{};
  File file;
  file.f = std::fopen(path.c_str(), "rb");
  if (!file.f) return bad(err, path, 0, "cannot be opened");
  std::vector<std::string> sizes, types, counts;
  bool have_fields = false, have_size = false, have_type = false, have_count = false, have_width = false, have_height = false, have_points = false, have_data = false;
  int line_no = 0, size_line = 0, points_line = 0;
  std::string line;
  while (!have_data)
  {
    line.clear();
    int ch;
    while ((ch = std::fgetc(file.f)) != EOF && ch != '\n')
    {
      if (line.size() > 65536) return bad(err, path, line_no + 1, "header line too long");
      line.push_back((char)ch);
    }
    if (ch == EOF && line.empty()) break;
    ++line_no;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::istringstream is(line);
    std::string key;
    if (!(is >> key) || key[0] == '#') continue;
    std::vector<std::string> tok;
    for (std::string t; is >> t;) tok.push_back(t);
    auto one = [&](long long& v) { return tok.size() == 1 && parse_int(tok[0], v) && v >= 0; };
    if (key == "VERSION") continue;
    else if (key == "FIELDS" || key == "COLUMNS")
    {
      if (tok.empty()) return bad(err, path, line_no, "FIELDS names no field");
      for (const auto& t : tok)
      {
        Field f;
        f.name = t;
        h.fields.push_back(f);
      }
      have_fields = true;
    }
    else if (key == "SIZE") { sizes = tok; have_size = true; size_line = line_no; }
    else if (key == "TYPE") { types = tok; have_type = true; }
    else if (key == "COUNT") { counts = tok; have_count = true; }
    else if (key == "WIDTH") { if (!one(h.width)) return bad(err, path, line_no, "malformed WIDTH"); have_width = true; }
    else if (key == "HEIGHT") { if (!one(h.height)) return bad(err, path, line_no, "malformed HEIGHT"); have_height = true; }
    else if (key == "VIEWPOINT") continue;
    else if (key == "POINTS") { if (!one(h.points)) return bad(err, path, line_no, "malformed POINTS"); have_points = true; points_line = line_no; }
    else if (key == "DATA")
    {
      if (tok.size() != 1) return bad(err, path, line_no, "malformed DATA");
      if (tok[0] == "ascii") h.format = kAscii;
      else if (tok[0] == "binary") h.format = kBinary;
      else if (tok[0] == "binary_compressed") h.format = kBinaryCompressed;
      else return bad(err, path, line_no, "unknown DATA format " + tok[0]);
      have_data = true;
      h.data_line = line_no;
      h.data_offset = std::ftell(file.f);
    }
    else return bad(err, path, line_no, "unknown header entry " + key);
  }
  if (!have_data) return bad(err, path, line_no, "the header has no DATA entry");
  if (!have_fields || !have_size || !have_type) return bad(err, path, h.data_line, "the header lacks FIELDS, SIZE or TYPE");
  const size_t nf = h.fields.size();
  if (sizes.size() != nf || types.size() != nf || (have_count && counts.size() != nf))
    return bad(err, path, size_line, "SIZE, TYPE and COUNT do not add up to the " + std::to_string(nf) + " FIELDS");
  int offset = 0;
  for (size_t i = 0; i < nf; ++i)
  {
    Field& f = h.fields[i];
    long long s = 0, c = 1;
    if (!parse_int(sizes[i], s) || (s != 1 && s != 2 && s != 4 && s != 8)) return bad(err, path, size_line, "SIZE " + sizes[i] + " of field " + f.name);
    if (types[i].size() != 1 || (types[i][0] != 'F' && types[i][0] != 'I' && types[i][0] != 'U')) return bad(err, path, size_line, "TYPE " + types[i] + " of field " + f.name);
    if (types[i][0] == 'F' && s < 4) return bad(err, path, size_line, "TYPE F of SIZE " + sizes[i] + " of field " + f.name);
    if (have_count && (!parse_int(counts[i], c) || c < 0 || c > (1 << 20))) return bad(err, path, size_line, "COUNT " + counts[i] + " of field " + f.name);
    f.size = (int)s;
    f.type = types[i][0];
    f.count = (int)c;
    f.offset = offset;
    if ((long long)offset + s * c > (1 << 24)) return bad(err, path, size_line, "records of more than 16 MiB");
    offset += (int)(s * c);
  }
  h.record_bytes = offset;
  if (offset == 0) return bad(err, path, size_line, "records of no bytes: every field has COUNT 0");
  if (!have_width && !have_points) return bad(err, path, h.data_line, "the header has neither WIDTH nor POINTS");
  if (!have_height) h.height = 1;
  if (!have_width) h.width = h.points;
  if (!have_points) h.points = h.width * h.height;
  if (h.points != h.width * h.height)
    return bad(err, path, points_line, "POINTS " + std::to_string(h.points) + " is not WIDTH * HEIGHT = " + std::to_string(h.width * h.height));
  if (h.points > 0x7fffffff) return bad(err, path, points_line, "more than 2^31 - 1 points");
  return LSA_OK;
}

ColumnTable table_of(const Header& h, bool columns, long long n)
{
  ColumnTable t;
  std::memset(&t, 0, sizeof(t));
  long long column_base = 0;
  for (const Field& f : h.fields)
  {
    // the first field of a name counts, with COUNT 1 only: every other one is skipped by its width
    for (int k = 0; k < kNbColumns && f.count == 1; ++k)
      if (f.name == kFieldNames[k] && t.c[k].type == kAbsent)
      {
        Column& c = t.c[k];
        c.base = columns ? column_base : f.offset;
        c.step = columns ? f.size : h.record_bytes;
        c.size = (uint8_t)f.size;
        c.type = f.type == 'F' ? kFloat : f.type == 'I' ? kSigned : kUnsigned;
      }
    column_base += (long long)f.size * f.count * n;
  }
  return t;
}

namespace
{
// one ascii row's tokens into the record the header declares
bool parse_row(const Header& h, const char*& p, const char* end, unsigned char* rec)
{
  for (const Field& f : h.fields)
    for (int c = 0; c < f.count; ++c)
    {
      while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) ++p;
      if (p >= end) return false;
      char* stop = nullptr;
      unsigned char* dst = rec + f.offset + c * f.size;
      if (f.type == 'F')
      {
        if (f.size == 4) { const float v = std::strtof(p, &stop); std::memcpy(dst, &v, 4); }
        else { const double v = std::strtod(p, &stop); std::memcpy(dst, &v, 8); }
      }
      else if (f.type == 'I') { const long long v = std::strtoll(p, &stop, 10); std::memcpy(dst, &v, f.size); }
      else { const unsigned long long v = std::strtoull(p, &stop, 10); std::memcpy(dst, &v, f.size); }
      if (stop == p) return false;
      p = stop;
    }
  return true;
}
}  // namespace

namespace
{
int read_cloud_unguarded(const std::string& path, Cloud& c, std::string& err, bool raw_binary);
}
int read_cloud(const std::string& path, Cloud& c, std::string& err, bool raw_binary)
{
  try { return read_cloud_unguarded(path, c, err, raw_binary); }
  catch (const std::bad_alloc&) { return bad(err, path, 0, "not enough memory for the data section"); }
}
namespace
{
int read_cloud_unguarded(const std::string& path, Cloud& c, std::string& err, bool raw_binary)
{
  timing() = Timing{};
  int rc = read_header(path, c.header, err);
  if (rc) return rc;
  const Header& h = c.header;
  const long long n = h.points;
  c.columns = h.format == kBinaryCompressed;
  c.table = table_of(h, c.columns, n);
  c.data.clear();
  if (n == 0) return LSA_OK;
  File file;
  file.f = std::fopen(path.c_str(), "rb");
  if (!file.f || std::fseek(file.f, (long)h.data_offset, SEEK_SET) != 0) return bad(err, path, 0, "cannot be read");
  const size_t raw = (size_t)n * h.record_bytes;
  // what the header promises is held against the file's size before anything of that size is allocated
  std::fseek(file.f, 0, SEEK_END);
  const long long section = std::max(0LL, (long long)std::ftell(file.f) - h.data_offset);
  std::fseek(file.f, (long)h.data_offset, SEEK_SET);
  if (h.format == kBinary && (unsigned long long)section < raw)
    return bad(err, path, h.data_line, "the data section is truncated: " + std::to_string(raw) + " bytes expected, " + std::to_string(section) + " there");
  if (h.format == kAscii && section < n)  // (a row is a character and a line end at the least)
    return bad(err, path, h.data_line, "the data section is truncated: " + std::to_string(n) + " rows expected in " + std::to_string(section) + " bytes");
  if (h.format == kBinaryCompressed && (unsigned long long)section * 264 < raw)  // (an LZF reference of three bytes stands for 264 at the most)
    return bad(err, path, h.data_line, "the data section is truncated: " + std::to_string(section) + " bytes cannot hold " + std::to_string(raw));
  double t0 = now_s();
  if (h.format == kBinary)
  {
    if (!raw_binary) return LSA_OK;  // the caller streams the records itself
    c.data.resize(raw);
    if (std::fread(c.data.data(), 1, raw, file.f) != raw) return bad(err, path, h.data_line, "the data section is truncated: " + std::to_string(raw) + " bytes expected");
    timing().file = now_s() - t0;
    return LSA_OK;
  }
  std::vector<unsigned char> body;
  {
    body.resize((size_t)section + 1);
    if (section > 0 && std::fread(body.data(), 1, (size_t)section, file.f) != (size_t)section) return bad(err, path, 0, "cannot be read");
    body[(size_t)section] = 0;  // strtof and its kin stop here: the text may end in a digit
  }
  timing().file = now_s() - t0;
  t0 = now_s();
  if (h.format == kAscii)
  {
    c.data.assign(raw, 0);
    const char* p = reinterpret_cast<const char*>(body.data());
    const char* end = p + body.size() - 1;
    for (long long i = 0; i < n; ++i)
      if (!parse_row(h, p, end, c.data.data() + (size_t)i * h.record_bytes))
        return bad(err, path, h.data_line + 1 + (int)i, "the data section is truncated or malformed: row " + std::to_string(i) + " of " + std::to_string(n));
    timing().text = now_s() - t0;
    return LSA_OK;
  }
  body.pop_back();
  if (body.size() < 8) return bad(err, path, h.data_line, "the data section is truncated: no compressed and raw sizes");
  uint32_t csize, usize;
  std::memcpy(&csize, body.data(), 4);
  std::memcpy(&usize, body.data() + 4, 4);
  if (usize != raw) return bad(err, path, h.data_line, "the raw size " + std::to_string(usize) + " is not POINTS * record size = " + std::to_string(raw));
  if (body.size() - 8 < csize) return bad(err, path, h.data_line, "the data section is truncated: " + std::to_string(csize) + " compressed bytes expected");
  c.data.resize(raw);
  const long long got = lzf_decompress(body.data() + 8, csize, c.data.data(), raw);
  if (got != (long long)raw) return bad(err, path, h.data_line, "the LZF stream does not decode to " + std::to_string(raw) + " bytes");
  timing().lzf = now_s() - t0;
  return LSA_OK;
}

}  // namespace

int read_points(const std::string& path, std::vector<lsa_point_t>& out, std::string& err)
{
  Cloud c;
  const int rc = read_cloud(path, c, err);
  if (rc) return rc;
  try { out.resize((size_t)c.header.points); }
  catch (const std::bad_alloc&) { return bad(err, path, 0, "not enough memory for the points"); }
  for (long long i = 0; i < c.header.points; ++i) out[(size_t)i] = decode_point(c.data.data(), c.table, i);
  return LSA_OK;
}

int read_normals(const std::string& path, std::vector<float>& out4, std::string& err)
{
  Cloud c;
  const int rc = read_cloud(path, c, err);
  if (rc) return rc;
  for (int k = kNormalX; k < kNbColumns; ++k)
  {
    const Column& col = c.table.c[k];
    if (col.type == kAbsent) return bad(err, path, 0, std::string("no field ") + kFieldNames[k] + " (of COUNT 1)");
    if (col.type != kFloat || col.size != 4) return bad(err, path, 0, std::string("the field ") + kFieldNames[k] + " is not a 4-byte F");
  }
  try { out4.resize((size_t)c.header.points * 4); }
  catch (const std::bad_alloc&) { return bad(err, path, 0, "not enough memory for the normals"); }
  for (long long i = 0; i < c.header.points; ++i)
    for (int k = 0; k < 4; ++k)
    {
      // (the bytes as they are: a NaN keeps its bits)
      const Column& col = c.table.c[kNormalX + k];
      std::memcpy(&out4[(size_t)i * 4 + k], c.data.data() + col.base + i * col.step, 4);
    }
  return LSA_OK;
}

namespace
{
void records_to_columns(const unsigned char* rec, long long n, unsigned char* col)
{
  int off = 0;
  for (int k = 0; k < kNbFields; ++k)
  {
    const int s = kFieldSizes[k];
    for (long long i = 0; i < n; ++i) std::memcpy(col + (size_t)i * s, rec + (size_t)i * kRecordBytes + off, s);
    col += (size_t)n * s;
    off += s;
  }
}
}  // namespace

int write_records(const std::string& path, const unsigned char* records, const unsigned char* columns, long long n, int format, std::string& err,
                  const float* normals4)
{
  timing() = Timing{};
  if (n <= 0) return -3;
  if (format < kAscii || format > kBinaryCompressed)
  {
    err = path + ": unknown PCD format " + std::to_string(format);
    return -4;
  }
  if (!records && !(columns && format == kBinaryCompressed)) return bad(err, path, 0, "no points given");
  const int nfields = normals4 ? (int)kNbColumns : (int)kNbFields;
  const int record_bytes = normals4 ? kRecordBytes + kNormalBytes : kRecordBytes;
  std::string head = "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS";
  for (int k = 0; k < nfields; ++k) head += std::string(" ") + kFieldNames[k];
  head += "\nSIZE";
  for (int k = 0; k < nfields; ++k) head += " " + std::to_string(kFieldSizes[k]);
  head += "\nTYPE";
  for (int k = 0; k < nfields; ++k) head += std::string(" ") + kFieldTypes[k];
  head += "\nCOUNT";
  for (int k = 0; k < nfields; ++k) head += " 1";
  head += "\nWIDTH " + std::to_string(n) + "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " + std::to_string(n) + "\nDATA ";
  head += format == kAscii ? "ascii\n" : format == kBinary ? "binary\n" : "binary_compressed\n";
  std::vector<unsigned char> body;
  const unsigned char* out = records;
  size_t out_bytes = (size_t)n * record_bytes;
  double t0 = now_s();
  if (format == kBinary && normals4)
  {
    // the 16 bytes of every normal behind the 28 of its point
    body.resize(out_bytes);
    for (long long i = 0; i < n; ++i)
    {
      std::memcpy(body.data() + (size_t)i * record_bytes, records + (size_t)i * kRecordBytes, kRecordBytes);
      std::memcpy(body.data() + (size_t)i * record_bytes + kRecordBytes, normals4 + (size_t)i * 4, kNormalBytes);
    }
    out = body.data();
  }
  if (format == kAscii)
  {
    // nine and seventeen significant digits: a float and a double read back to the same bits
    std::string text;
    text.reserve((size_t)n * 96);
    char row[256];
    for (long long i = 0; i < n; ++i)
    {
      const unsigned char* r = records + (size_t)i * kRecordBytes;
      float x, y, z, in;
      double t;
      uint16_t laser;
      std::memcpy(&x, r, 4); std::memcpy(&y, r + 4, 4); std::memcpy(&z, r + 8, 4); std::memcpy(&t, r + 12, 8); std::memcpy(&in, r + 20, 4); std::memcpy(&laser, r + 24, 2);
      int len = std::snprintf(row, sizeof(row), "%.9g %.9g %.9g %.17g %.9g %u %u %u", x, y, z, t, in, (unsigned)laser, (unsigned)r[26], (unsigned)r[27]);
      for (int k = 0; normals4 && k < 4; ++k)
      {
        // a voxel without a normal is spelled nan, whatever the C library makes of the sign
        const float v = normals4[(size_t)i * 4 + k];
        len += v != v ? std::snprintf(row + len, sizeof(row) - (size_t)len, " nan") : std::snprintf(row + len, sizeof(row) - (size_t)len, " %.9g", v);
      }
      row[len++] = '\n';
      text.append(row, (size_t)len);
    }
    body.assign(text.begin(), text.end());
    out = body.data();
    out_bytes = body.size();
    timing().text = now_s() - t0;
  }
  else if (format == kBinaryCompressed)
  {
    if ((unsigned long long)out_bytes > 0xffffffffull) return bad(err, path, 0, "more than 4 GiB do not fit the compressed format's sizes");
    std::vector<unsigned char> made;
    if (!columns || normals4)
    {
      made.resize(out_bytes);
      if (columns) std::memcpy(made.data(), columns, (size_t)n * kRecordBytes);
      else records_to_columns(records, n, made.data());
      // the four columns of the normals behind the eight
      for (int k = 0; normals4 && k < 4; ++k)
        for (long long i = 0; i < n; ++i) std::memcpy(made.data() + (size_t)n * kRecordBytes + ((size_t)k * n + (size_t)i) * 4, normals4 + (size_t)i * 4 + k, 4);
      columns = made.data();
    }
    const std::vector<unsigned char> z = lzf_compress(columns, out_bytes);
    const uint32_t csize = (uint32_t)z.size(), usize = (uint32_t)out_bytes;
    body.resize(8 + z.size());
    std::memcpy(body.data(), &csize, 4);
    std::memcpy(body.data() + 4, &usize, 4);
    std::memcpy(body.data() + 8, z.data(), z.size());
    out = body.data();
    out_bytes = body.size();
    timing().lzf = now_s() - t0;
  }
  t0 = now_s();
  File file;
  file.f = std::fopen(path.c_str(), "wb");
  if (!file.f) return bad(err, path, 0, "cannot be written");
  const bool ok = std::fwrite(head.data(), 1, head.size(), file.f) == head.size() && std::fwrite(out, 1, out_bytes, file.f) == out_bytes;
  const bool closed = std::fclose(file.f) == 0;
  file.f = nullptr;
  if (!ok || !closed) return bad(err, path, 0, "cannot be written");
  timing().file = now_s() - t0;
  return LSA_OK;
}

int write_points(const std::string& path, const lsa_point_t* pts, long long n, int format, std::string& err)
{
  if (n <= 0) return -3;
  if (!pts) return bad(err, path, 0, "no points given");
  std::vector<unsigned char> rec((size_t)n * kRecordBytes);
  for (long long i = 0; i < n; ++i)
  {
    uint32_t w[7];
    encode_record(pts[i], w);
    std::memcpy(rec.data() + (size_t)i * kRecordBytes, w, kRecordBytes);
  }
  return write_records(path, rec.data(), nullptr, n, format, err);
}

// ---- LZF --------------------------------------------------------------------------------------------------------------
// back references reach 8192 bytes back and copy 3 to 264 bytes; a hash of the next three bytes finds the candidate
std::vector<unsigned char> lzf_compress(const unsigned char* in, size_t n)
{
  constexpr int kHashBits = 16;
  constexpr size_t kMaxOff = 1 << 13, kMaxRef = (1 << 8) + (1 << 3), kMaxLit = 1 << 5;
  std::vector<unsigned char> out;
  out.reserve(n / 2 + 16);
  std::vector<long long> table((size_t)1 << kHashBits, -1);
  size_t lit_start = 0, i = 0;
  auto flush = [&](size_t end) {
    while (lit_start < end)
    {
      const size_t run = std::min(end - lit_start, kMaxLit);
      out.push_back((unsigned char)(run - 1));
      out.insert(out.end(), in + lit_start, in + lit_start + run);
      lit_start += run;
    }
  };
  while (i + 2 < n)
  {
    const uint32_t v = (uint32_t)in[i] | ((uint32_t)in[i + 1] << 8) | ((uint32_t)in[i + 2] << 16);
    const uint32_t hsh = (v * 2654435761u) >> (32 - kHashBits);
    const long long ref = table[hsh];
    table[hsh] = (long long)i;
    if (ref >= 0 && i - (size_t)ref <= kMaxOff && in[ref] == in[i] && in[ref + 1] == in[i + 1] && in[ref + 2] == in[i + 2])
    {
      size_t len = 3;
      const size_t max_len = std::min(kMaxRef, n - i);
      while (len < max_len && in[ref + len] == in[i + len]) ++len;
      flush(i);
      const size_t off = i - (size_t)ref - 1, l = len - 2;
      if (l < 7) out.push_back((unsigned char)((l << 5) | (off >> 8)));
      else
      {
        out.push_back((unsigned char)((7 << 5) | (off >> 8)));
        out.push_back((unsigned char)(l - 7));
      }
      out.push_back((unsigned char)(off & 0xff));
      i += len;
      lit_start = i;
    }
    else ++i;
  }
  flush(n);
  return out;
}

long long lzf_decompress(const unsigned char* in, size_t n, unsigned char* out, size_t capacity)
{
  size_t ip = 0, op = 0;
  while (ip < n)
  {
    const unsigned c = in[ip++];
    if (c < 32)
    {
      const size_t run = c + 1;
      if (ip + run > n || op + run > capacity) return -1;
      std::memcpy(out + op, in + ip, run);
      ip += run;
      op += run;
    }
    else
    {
      size_t len = c >> 5;
      if (len == 7)
      {
        if (ip >= n) return -1;
        len += in[ip++];
      }
      len += 2;
      if (ip >= n) return -1;
      const size_t off = ((size_t)(c & 31) << 8 | in[ip++]) + 1;
      if (off > op || op + len > capacity) return -1;
      for (size_t k = 0; k < len; ++k, ++op) out[op] = out[op - off];  // byte by byte: a reference may overlap what it writes
    }
  }
  return (long long)op;
}

}  // namespace pcd
}  // namespace lsa

// ---- C exports (host only, no device needed) ----------------------------------------------------------------------------
namespace
{
std::string& pcd_error()
{
  thread_local std::string e;
  return e;
}
}  // namespace

extern "C" {

const char* lsa_pcd_last_error(void) { return pcd_error().c_str(); }

int lsa_pcd_info(const char* path, int* n, int* format)
{
  if (!path) return LSA_E_ARG;
  lsa::pcd::Header h;
  const int rc = lsa::pcd::read_header(path, h, pcd_error());
  if (rc) return rc;
  if (n) *n = (int)h.points;
  if (format) *format = h.format;
  return LSA_OK;
}

int lsa_pcd_read(const char* path, lsa_point_t* out, int capacity)
{
  if (!path || capacity < 0 || (capacity > 0 && !out)) return LSA_E_ARG;
  std::vector<lsa_point_t> pts;
  const int rc = lsa::pcd::read_points(path, pts, pcd_error());  // (reports a file too large for the memory itself)
  if (rc) return rc;
  const size_t n = std::min(pts.size(), (size_t)capacity);
  if (n > 0) std::memcpy(out, pts.data(), n * sizeof(lsa_point_t));
  return (int)pts.size();
}

int lsa_pcd_read_normals(const char* path, float* out4, int capacity)
{
  if (!path || capacity < 0 || (capacity > 0 && !out4)) return LSA_E_ARG;
  std::vector<float> normals;
  const int rc = lsa::pcd::read_normals(path, normals, pcd_error());
  if (rc) return rc;
  const size_t n = std::min(normals.size() / 4, (size_t)capacity);
  if (n > 0) std::memcpy(out4, normals.data(), n * 4 * sizeof(float));
  return (int)(normals.size() / 4);
}

int lsa_pcd_write(const char* path, const lsa_point_t* pts, int n, int format)
{
  if (!path || n < 0) return LSA_E_ARG;
  try { return lsa::pcd::write_points(path, pts, n, format, pcd_error()); }
  catch (const std::bad_alloc&) { pcd_error() = std::string(path) + ": not enough memory"; return LSA_E_CAPACITY; }
}

int lsa_lzf_compress(const void* in, size_t n, void* out, size_t capacity, size_t* written)
{
  if ((!in && n > 0) || !written) return LSA_E_ARG;
  const std::vector<unsigned char> z = lsa::pcd::lzf_compress(static_cast<const unsigned char*>(in), n);
  *written = z.size();
  if (z.size() > capacity || (!out && !z.empty())) return LSA_E_CAPACITY;
  if (!z.empty()) std::memcpy(out, z.data(), z.size());
  return LSA_OK;
}

int lsa_lzf_decompress(const void* in, size_t n, void* out, size_t capacity, size_t* written)
{
  if ((!in && n > 0) || (!out && capacity > 0) || !written) return LSA_E_ARG;
  const long long got = lsa::pcd::lzf_decompress(static_cast<const unsigned char*>(in), n, static_cast<unsigned char*>(out), capacity);
  if (got < 0) return LSA_E_ARG;
  *written = (size_t)got;
  return LSA_OK;
}

}  // extern "C"
