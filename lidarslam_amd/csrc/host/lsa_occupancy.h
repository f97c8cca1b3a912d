// lsa_occupancy.h -- the 2-D occupancy grid of the dense map's floor plan as map_server reads it (internal, host only):
// <prefix>.pgm, binary P5 of maxval 255, image row 0 the grid's last row, and <prefix>.yaml beside it.
#pragma once
#include <cstdint>
#include <string>
#include "../../../include/lidarslam_amd.h"

namespace lsa
{
namespace occupancy
{
constexpr unsigned char kOccupiedGrey = 0, kFreeGrey = 254, kUnknownGrey = 205;

// the grey level of a state: 100 occupied, 0 free, anything else unknown
inline unsigned char grey_of(int8_t state) { return state == 100 ? kOccupiedGrey : (state == 0 ? kFreeGrey : kUnknownGrey); }

// writes both files; the number of cells (0 and no file for a grid without cells), or LSA_E_ARG with the reason in err
long long write(const std::string& prefix, const lsa_dense_grid_info_t& info, const int8_t* state, std::string& err);
}  // namespace occupancy
}  // namespace lsa
