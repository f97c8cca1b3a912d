// lsa_place.h -- the host statement of place recognition on the keypoint log: a frame's descriptor, the distance of two
// descriptors, and the selection of candidates on a trajectory.  The descriptor's and the distance's arithmetic is
// ../lsa_scan_descriptor.h's, the text the device compiles too (lsa_place.hip); the loops around it here are the plain
// sequential ones the device's results are held to, byte for byte.  No device, no state: a stand-alone program runs them
// under the sanitizers (tests/place_sanitize.cpp).
#pragma once
#include "../lsa_place_select.h"
#include "../lsa_scan_descriptor.h"

namespace lsa
{
namespace host
{
// rings * sectors + sectors floats from n points (the caller has filtered them by type); LSA_E_ARG for bad parameters
int ScanDescriptor(const lsa_place_params_t& p, const lsa_point_t* pts, int n, float* out);
// query a against candidate b: the smallest distance over the column shifts and its shift, the lowest on a tie
int PlaceDistance(const lsa_place_params_t& p, const float* a, const float* b, float* distance, int* shift);
// lsa_place_select_host (include/lidarslam_amd.h)
int PlaceSelect(const float* distance, const int32_t* shift, const double* poses17, int n, int query, int sectors, double minTravelled, double maxDistance,
                double maxDescriptorDistance, int exclusionHalfWindow, lsa_place_candidate_t* out, int capacity);
// lsa_place_detect_host (include/lidarslam_amd.h): the loop over PlaceDistance and PlaceSelect, query by query
int PlaceDetect(const lsa_loop_detect_t& detect, const float* descriptors, const double* poses17, int n, lsa_loop_candidate_t* out, int capacity);
// what the device's selection reads of the trajectory (../lsa_place_select.h): positions, and travelled[] as PlaceSelect sums it
void FramePositions(const double* poses17, int n, place::FramePosition* out);
// the detection's argument check: the number of queries (>= 1) with *last the resolved last query, or LSA_E_ARG
int DetectQueries(const lsa_loop_detect_t& detect, int n, int capacity, int* last);
// the descriptor of a map as seen from a viewpoint (lsa_scan_descriptor.h: map_coord): ScanDescriptor of the translated points
int MapDescriptor(const lsa_place_params_t& p, const lsa_point_t* pts, int n, const double viewpoint[3], float* out);
// lsa_map_place_select_host (include/lidarslam_amd.h)
bool MapSearchOk(const lsa_map_place_search_t& s);
int MapPlaceSelect(const float* distance, const int32_t* shift, const double* viewpoints, int V, int sectors, const lsa_map_place_search_t& s,
                   lsa_map_place_candidate_t* out, int capacity);
}  // namespace host
}  // namespace lsa
