// lsa_device_grid_io.h -- what the map-file unit (lsa_pcd.hip) and the keypoint log's replay (lsa_kplog.hip) need of a device
// grid: the batch buffer an insertion reads and the insertion itself (lsa_grid_add.hip), RollingGrid::Get left on the device
// (lsa_grid_submap.hip).  What the grid's own units share is lsa_grid.h.
#pragma once
#include "lsa_ctx.h"

namespace lsa
{
lsa_ctx* grid_context(lsa_device_grid* g);
hipStream_t grid_stream(lsa_device_grid* g);
int grid_batch(lsa_device_grid* g, int n, lsa_point_t** batch);
int grid_add_batch(lsa_device_grid* g, int n, bool fixed, double time, bool do_roll);
int grid_collect(lsa_device_grid* g, int clean, const lsa_point_t** pts, int* n);
int pcd_save_device_points(lsa_ctx* ctx, hipStream_t gs, const lsa_point_t* pts, int n, const char* path, int format, const float* normals4 = nullptr);  // lsa_pcd.hip: points written, 0 and no file for none
int grid_adopt_parameters(lsa_device_grid* dst, const lsa_device_grid* src);  // lsa_device_grid.hip: dst emptied, with src's geometry, sampling mode and order
}  // namespace lsa
