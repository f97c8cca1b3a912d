// lsa_map_order.h -- the iteration order of LidarSlam::RollingGrid's containers for a map whose points live elsewhere
// (the device grid, lsa_grid_order.hip, with "Ordered" = 0).
//
// The reference's Get / BuildSubMapKdTree hand the voxels out in the iteration order of
// std::unordered_map<int, std::unordered_map<int, Voxel>> (RollingGrid.cxx:95-113, 362-442): an accident of the tables'
// history -- which keys came in which order, which were erased, when a table rehashed, that clear() keeps the bucket
// array.  KeyShadow holds the same two levels of tables with the keys alone and applies the same sequence of container
// operations RollingGrid.cxx applies, so its iteration order IS the reference's, by construction and not by a model of
// the library.  The device grid records what each of its modifications did to the key set (lsa_grid_order.hip) and
// replays it here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <unordered_map>
#include <vector>

namespace lsa
{
namespace host
{

class KeyShadow
{
public:
  using Key = unsigned long long;  // outer index << 32 | leaf index, both as unsigned (the device grid's key)
  // the value is never read: only the tables' structure matters
  using Inner = std::unordered_map<int, unsigned char>;
  using Outer = std::unordered_map<int, Inner>;

  // RollingGrid::Clear (:51-56), also through Reset (:40-48): the bucket arrays stay
  void Clear()
  {
    Voxels.clear();
    Count = 0;
  }
  // tables never used (a grid that switches to this order while it holds points starts from these)
  void Fresh()
  {
    Outer().swap(Voxels);
    Count = 0;
  }
  // Roll (:136-156): a fresh outer table, filled in the iteration order of the old one, the inner tables moved
  void Roll(const int off[3], int gridSize)
  {
    if (!off[0] && !off[1] && !off[2]) return;  // (:128-134: no move, nothing is rebuilt)
    std::size_t kept = 0;
    Outer rolled;
    for (auto& o : Voxels)
    {
      int id = o.first;
      const int z = id / (gridSize * gridSize);
      id -= z * gridSize * gridSize;
      const int y = id / gridSize;
      const int x = id - y * gridSize;
      const int v[3] = {x - off[0], y - off[1], z - off[2]};
      if (v[0] < 0 || v[1] < 0 || v[2] < 0 || v[0] >= gridSize || v[1] >= gridSize || v[2] >= gridSize) continue;
      kept += o.second.size();
      rolled[v[2] * gridSize * gridSize + v[1] * gridSize + v[0]] = std::move(o.second);
    }
    Voxels.swap(rolled);
    Count = kept;
  }
  // Add (:206-212): Voxels[idxOut][idxIn] for a key not in the map (the outer voxel first if it is new)
  void Insert(Key key)
  {
    Voxels[static_cast<int>(static_cast<unsigned>(key >> 32))][static_cast<int>(static_cast<unsigned>(key))];
    ++Count;
  }
  // ClearOldPoints (:325-350): the leaves in `erased` (sorted) go, in the iteration order, and every outer voxel left
  // empty goes with its last leaf
  void Erase(const std::vector<Key>& erased)
  {
    for (auto out = Voxels.begin(); out != Voxels.end();)
    {
      const Key hi = static_cast<Key>(static_cast<unsigned>(out->first)) << 32;
      for (auto in = out->second.begin(); in != out->second.end();)
      {
        if (std::binary_search(erased.begin(), erased.end(), hi | static_cast<unsigned>(in->first)))
        {
          in = out->second.erase(in);
          --Count;
        }
        else ++in;
      }
      if (out->second.empty()) out = Voxels.erase(out);
      else ++out;
    }
  }
  std::size_t Size() const { return Count; }
  // the keys (outer index << 32 | leaf index, both as unsigned) in iteration order
  void Keys(Key* out) const
  {
    for (const auto& o : Voxels)
    {
      const Key hi = static_cast<Key>(static_cast<unsigned>(o.first)) << 32;
      for (const auto& i : o.second) *out++ = hi | static_cast<unsigned>(i.first);
    }
  }

private:
  Outer Voxels;
  std::size_t Count = 0;
};

}  // namespace host
}  // namespace lsa
