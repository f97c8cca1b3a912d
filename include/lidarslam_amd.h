/*
 * lidarslam_amd.h -- C ABI of liblidarslam_amd.so: the MI355X-native
 * implementation of the per-frame scan-matching hot path of
 * Perception4D/LidarSlam (slam_lib).
 *
 * The reference has no FFI layer: the path sits behind the C++ API of
 * libLidarSlam.  This header is the seam a maintainer binds
 * instead of the four internal call sites listed below.  Plain pointers and
 * sizes only -- no STL / Eigen / PCL / torch types cross this boundary.  All
 * device memory is owned by the context; the host never sees device pointers.
 *
 * All functions return 0 on success and a negative LSA_E_* code on failure;
 * lsa_last_error() returns a human readable message for the last failure of
 * that context.  There is NO CPU fallback: when no HIP device is usable,
 * lsa_ctx_create fails with LSA_E_NO_DEVICE and nothing else can be called.
 *
 * file:line citations are relative to /root/reference.
 */
#ifndef LIDARSLAM_AMD_H
#define LIDARSLAM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSA_OK 0
#define LSA_E_NO_DEVICE (-1)
#define LSA_E_HIP (-2)
#define LSA_E_ARG (-3)
#define LSA_E_STATE (-4)
#define LSA_E_CAPACITY (-5)

/* Keypoint types -- slam_lib/include/LidarSlam/Enums.h:30-36 */
#define LSA_EDGE 0
#define LSA_PLANE 1
#define LSA_BLOB 2

/* The 32-byte PCL point of the reference, byte for byte
 * -- slam_lib/include/LidarSlam/LidarPoint.h:31-64 (registered :68-77). */
typedef struct lsa_point_t
{
  float x, y, z, w;   /* PCL_ADD_POINT4D: data[4], w == 1 */
  double time;        /* offset in seconds to the frame stamp */
  float intensity;
  uint16_t laser_id;  /* ring, 0 = lowest */
  uint8_t device_id;
  uint8_t label;
} lsa_point_t;

/* Match status values -- slam_lib/include/LidarSlam/KeypointsMatcher.h:82-93 */
enum
{
  LSA_MATCH_SUCCESS = 0,
  LSA_MATCH_BAD_MODEL_PARAMETRIZATION = 1,
  LSA_MATCH_NOT_ENOUGH_NEIGHBORS = 2,
  LSA_MATCH_NEIGHBORS_TOO_FAR = 3,
  LSA_MATCH_BAD_PCA_STRUCTURE = 4,
  LSA_MATCH_INVALID_NUMERICAL = 5,
  LSA_MATCH_MSE_TOO_LARGE = 6,
  LSA_MATCH_UNKOWN = 7,
  LSA_MATCH_NSTATUS = 8
};

/* Parameters of SpinningSensorKeypointExtractor, same names and defaults as its
 * setters -- slam_lib/include/LidarSlam/SpinningSensorKeypointExtractor.h:44-70, 125-157 */
typedef struct lsa_extract_params_t
{
  int32_t neighbor_width;            /* NeighborWidth = 4 */
  float min_distance_to_sensor;      /* MinDistanceToSensor = 1.5 m */
  float min_beam_surface_angle;      /* MinBeamSurfaceAngle = 10 deg */
  float plane_sin_angle_threshold;   /* PlaneSinAngleThreshold = 0.5 */
  float edge_sin_angle_threshold;    /* EdgeSinAngleThreshold = 0.86 */
  float dist_to_line_threshold;      /* DistToLineThreshold = 0.20 m */
  float edge_depth_gap_threshold;    /* EdgeDepthGapThreshold = 0.15 m */
  float edge_saliency_threshold;     /* EdgeSaliencyThreshold = 1.5 m */
  float edge_intensity_gap_threshold;/* EdgeIntensityGapThreshold = 50 */
} lsa_extract_params_t;

/* KeypointsMatcher::Parameters -- slam_lib/include/LidarSlam/KeypointsMatcher.h:43-77 */
typedef struct lsa_match_params_t
{
  int32_t single_edge_per_ring;      /* SingleEdgePerRing */
  int32_t edge_nb_neighbors;         /* EdgeNbNeighbors */
  int32_t edge_min_nb_neighbors;     /* EdgeMinNbNeighbors */
  int32_t plane_nb_neighbors;        /* PlaneNbNeighbors */
  int32_t blob_nb_neighbors;         /* BlobNbNeighbors */
  int32_t reserved;
  double max_neighbors_distance;     /* MaxNeighborsDistance */
  double edge_max_model_error;       /* EdgeMaxModelError */
  double planarity_threshold;        /* PlanarityThreshold */
  double plane_max_model_error;      /* PlaneMaxModelError */
  double saturation_distance;        /* SaturationDistance (Tukey scale) */
} lsa_match_params_t;

/* Which device-resident keypoint set an operation reads */
#define LSA_SET_RAW_CURRENT 0   /* Slam::CurrentRawKeypoints           (Slam.h:516) */
#define LSA_SET_RAW_PREVIOUS 1  /* Slam::PreviousRawKeypoints          (Slam.h:517) */
#define LSA_SET_WORKING 2       /* Slam::CurrentUndistortedKeypoints   (Slam.h:520) */

/* ------------------------------------------------------------------------- */
/* Context: one per Slam instance, bound to one HIP device and one stream.    */
typedef struct lsa_ctx lsa_ctx;

int lsa_device_count(void);
int lsa_ctx_create(int device_id, lsa_ctx** out);
/* Restricts the calling thread (and the threads it creates afterwards: call it before lsa_ctx_create /
 * lsa_slam_create) to the CPUs of the NUMA node the device is attached to.  A frame is tens of short host <-> device
 * round trips (mailbox polls, pinned staging buffers); from the other socket of a two-socket host they take about
 * twice as long.  Returns the node (>= 0), LSA_E_STATE when the host has no NUMA information or none of the node's
 * CPUs may be used, LSA_E_NO_DEVICE for a bad device.  Optional: nothing else depends on it. */
int lsa_bind_host_to_device(int device_id);
void lsa_ctx_destroy(lsa_ctx* ctx);
const char* lsa_last_error(const lsa_ctx* ctx);
/* Blocks until everything queued on the context's stream has finished. */
int lsa_sync(lsa_ctx* ctx);

/* ------------------------------------------------------------------------- */
/* Seam 1: SpinningSensorKeypointExtractor::ComputeKeyPoints(pc)
 * -- slam_lib/src/SpinningSensorKeypointExtractor.cxx:118-136, called from
 *    Slam::ExtractKeypoints, slam_lib/src/Slam.cxx:784.                       */

/* Copies one scan (firing order, rings interleaved) to the device and makes it
 * the current frame.  On the first usable frame the azimuthal resolution is
 * estimated on the host exactly as EstimateAzimuthalResolution does
 * (SSKE.cxx:593-637) and then frozen in the context (SSKE.cxx:169-170). */
int lsa_upload_frame(lsa_ctx* ctx, const lsa_point_t* pts, int n);

/* The sensor driver's record layout (a sensor_msgs/PointCloud2 of velodyne_pcl::PointXYZIRT, or any record
 * with float x, y, z, intensity, time and a uint16 ring): byte offsets inside a record of point_step bytes. */
typedef struct lsa_wire_layout_t
{
  int32_t point_step;
  int32_t off_x, off_y, off_z, off_intensity, off_ring, off_time;
} lsa_wire_layout_t;

/* lsa_upload_frame for the driver's records, converted on the device as VelodyneToLidarNode::Callback does on
 * the host (ros_wrapping/lidar_conversions/src/VelodyneToLidarNode.cxx:52-112): laser_id = mapping[ring] (or
 * ring when mapping_len == 0), device_id, time = the record's time offset.  When the time field is not usable
 * (last - first <= 1e-8, :74) the time is built from the azimuth advancement exactly as the node does
 * (SpinningFrameAdvancementEstimator, lidar_conversions/src/Utilities.h:62-114, rpm and timestamp_first_packet
 * as its parameters): per ring, in arrival order, a point gets + 1 turn when the ring's last descent of the
 * advancement (a point below the ring's point right in front of it) lies behind the ring's last NaN advancement (a NaN
 * x or y: the node stores the NaN and the ring starts afresh) -- without NaN records that is "the first descent and
 * everything after it".  Both are scanned on the ring-bucketed frame on the device (portable arc tangent: the time
 * agrees with the node's to rounding; the arc tangent does not tell y = -0.0 from +0.0 at x < 0, where libm gives -pi
 * and +pi, and the wrap into [0, 1) makes the two advancements agree).  A laser id behind the mapping's end is 0xffff.
 * The first frame (azimuthal resolution estimate) and a frame with a laser id >= 512, which the bucketing cannot hold,
 * are converted on the host, with libm. */
int lsa_upload_wire_frame(lsa_ctx* ctx, const void* records, int n, const lsa_wire_layout_t* layout, const uint16_t* laser_id_mapping,
                          int mapping_len, int device_id, double rpm, int timestamp_first_packet);

/* lsa_upload_frame for the RoboSense driver's organized cloud (height = lasers, width = points per laser, row after row,
 * records of pcl::PointXYZI: float x, y, z, intensity at the given byte offsets -- off_ring and off_time of the layout are
 * not used), converted on the device as RobosenseToLidarNode::Callback does on the host
 * (ros_wrapping/lidar_conversions/src/RobosenseToLidarNode.cxx:58-125): records with a NaN or infinite coordinate are
 * dropped (:82-83); so is a record whose three coordinates equal those of the last point kept (second return of the dual
 * return mode, :87-88); laser_id = mapping[i / width], or RS16's own mapping when there are 16 lasers and no mapping is
 * given, or i / width (:106-109); time = ((i mod (size / height)) / (size / height) - 1) / rpm * 60 (:118-119); the points
 * kept stay in their order.  *n_valid = points kept (= the size of the current frame; 0 and no frame when none is). */
int lsa_upload_robosense_frame(lsa_ctx* ctx, const void* records, int width, int height, const lsa_wire_layout_t* layout, const uint16_t* laser_id_mapping,
                               int mapping_len, int device_id, double rpm, int* n_valid);

/* lsa_upload_frame for a LidarView / ParaView frame, converted on the device as vtkSlam::PolyDataToPointCloud does on the
 * host (paraview_wrapping/Plugin/vtkLidarSlam/vtkSlam.cxx:668-707), from the vtkPolyData's own arrays -- structure
 * of arrays, no LidarPoint cloud is built on the host: xyz = 3 n interleaved coordinates (vtkPoints, float or double),
 * time / laser_id / intensity = the point-data arrays named by the filter (any of the scalar types below).  The
 * frame's end is the largest time; *stamp_us = end * (time_to_seconds * 1e6), a point's time = (t - end) *
 * time_to_seconds, laser_id = mapping[id] (or id when mapping_len == 0); points whose three coordinates are all zero
 * are dropped, the others keep their order.  *n_valid = points kept (= the size of the current frame).  Returns 1
 * when every point was kept ("allPointsAreValid"), 0 when some were dropped, < 0 on error. */
enum { LSA_SCALAR_F32 = 0, LSA_SCALAR_F64 = 1, LSA_SCALAR_U8 = 2, LSA_SCALAR_U16 = 3, LSA_SCALAR_U32 = 4, LSA_SCALAR_I32 = 5 };
int lsa_upload_polydata_frame(lsa_ctx* ctx, int n, const void* xyz, int xyz_type, const void* time, int time_type, const void* laser_id, int laser_type,
                              const void* intensity, int intensity_type, const uint16_t* laser_id_mapping, int mapping_len, double time_to_seconds,
                              uint64_t* stamp_us, int* n_valid);

/* Frame store: keeps scans resident in HBM so that a replay (bench.py) can
 * time the path without the PCIe copy.  Slots are created on demand. */
int lsa_frame_store_put(lsa_ctx* ctx, int slot, const lsa_point_t* pts, int n);
int lsa_frame_store_use(lsa_ctx* ctx, int slot);

/* Number of points of the current frame. */
int lsa_frame_size(const lsa_ctx* ctx);
/* The current frame as the device holds it: a plain copy on the context's stream, waited for -- every bit as it is
 * (-0.0, NaN payloads; lsa_transform_frame with the identity keeps neither).  Returns the number of points,
 * LSA_E_STATE when there is no frame, LSA_E_CAPACITY when capacity is below the frame's size. */
int lsa_download_frame(lsa_ctx* ctx, lsa_point_t* out, int capacity);

float lsa_get_azimuthal_resolution(const lsa_ctx* ctx);
void lsa_set_azimuthal_resolution(lsa_ctx* ctx, float rad);

/* Runs a3-a8 of SURVEY.md 8a on the current frame.  The previous call's
 * keypoints become LSA_SET_RAW_PREVIOUS (Slam.cxx:751).  counts[k] = number of
 * keypoints of type k; keypoints stay on the device, ordered ring-major /
 * index-ascending as SSKE.cxx:575-589 pushes them.  A frame that is refused
 * (laser_id >= 512, more than 8192 points on one ring: LSA_E_CAPACITY) changes
 * neither set: the next frame's LSA_SET_RAW_PREVIOUS is the last frame that
 * was extracted. */
int lsa_extract_keypoints(lsa_ctx* ctx, const lsa_extract_params_t* params, int counts[3]);
/* A further frame of the same Slam::AddFrames call (another LiDAR device, Slam.cxx:753-801): the frame in the context
 * is extracted with `params` (and the azimuthal resolution set for that device) and its keypoints are appended to
 * the RAW_CURRENT sets instead of replacing them -- AggregateFrames(keypoints, false) (Slam.cxx:1512-1578):
 * time += time_offset, then the rigid transform sensor -> BASE (NULL = identity, coordinates untouched).
 * counts[] = keypoints of this frame per type. */
int lsa_extract_keypoints_more(lsa_ctx* ctx, const lsa_extract_params_t* params, const double base_to_lidar[16], double time_offset, int counts[3]);
/* A frame handed over AHEAD of the AddFrame call that will use it (offline / batch replay: the caller holds the
 * next cloud while the current one is being registered).  lsa_upload_frame_begin returns at once: a thread of the
 * context copies the (pageable) cloud into pinned staging memory and enqueues the DMA on a copy stream of its own,
 * into one of three device buffers, so that the upload of frame f + 1 runs beside the registration of frame f.
 * Up to two clouds may be announced before the first of them is used (the replay announces frame f + 1 just before it
 * adds frame f, which it announced one call earlier); a third announcement gives the oldest up.  `pts` must stay valid
 * and unchanged until the frame has been adopted or given up.
 * lsa_upload_frame_ready: 1 once the DMA of the OLDEST announced cloud has been enqueued (lsa_extract_prefetch_uploaded
 * may follow).  lsa_upload_frame_adopt(pts, n): makes an announced cloud the current frame (as lsa_upload_frame would)
 * when it is the very buffer that was announced -- returns 1; clouds announced before it are given up --, returns 0
 * when it was not announced (the caller then calls lsa_upload_frame).  lsa_extract_prefetch_uploaded:
 * lsa_extract_prefetch for the oldest announced cloud. */
int lsa_upload_frame_begin(lsa_ctx* ctx, const lsa_point_t* pts, int n);
int lsa_upload_frame_ready(const lsa_ctx* ctx);
int lsa_upload_frame_adopt(lsa_ctx* ctx, const lsa_point_t* pts, int n);
/* Page-locks a host buffer the caller hands clouds over in again and again (a driver's ring of scan buffers): uploads
 * from it (lsa_upload_frame, lsa_slam_add_frame) are then one DMA at the bus rate, asynchronous to the caller, instead of
 * a staged copy through the runtime's own pinned chunks (VLS-128, 8.2 MB: 0.15 ms against 0.3 ms).  Process-wide
 * (hipHostRegister); lsa_unpin_host_memory before the buffer is freed. */
int lsa_pin_host_memory(void* ptr, size_t bytes);
int lsa_unpin_host_memory(void* ptr);
/* Gives up every cloud announced with lsa_upload_frame_begin and not adopted yet (Slam::Reset: nothing announced before a
 * reset is taken over after it).  A cloud whose buffer was rewritten since it was announced is never adopted either: a
 * sample of its contents is compared (lsa_upload_frame_adopt then returns 0 and the caller uploads). */
int lsa_upload_frame_forget(lsa_ctx* ctx);
/* Frees the buffers the context has outgrown since the last call.  Growth never frees on the spot: hipFree waits for the
 * whole device with the runtime's lock held, which stalls every thread that enqueues, and retiring a buffer instead lets
 * growth go without a stream synchronise (launches in flight keep the old buffer).  The pipeline calls it at the start of
 * every AddFrame. */
int lsa_collect_garbage(lsa_ctx* ctx);
int lsa_uploads_adopted(const lsa_ctx* ctx);
int lsa_extract_prefetch_uploaded(lsa_ctx* ctx, const lsa_extract_params_t* params);
/* Look-ahead for replay from the frame store: extracts the keypoints of the frame in `slot` on a stream of its own,
 * beside whatever runs on the context's stream (the registration of the current frame), into spare buffers.  The
 * next lsa_extract_keypoints adopts them -- no kernel, no wait -- if it is called for that very frame
 * (lsa_frame_store_use(slot)) with the same parameters, keypoint types and azimuthal resolution; otherwise the
 * look-ahead is dropped and the extraction runs as usual.  Same keypoints either way (the extraction does not depend
 * on the pose).  Call it after the current frame's lsa_extract_keypoints; until the adoption lsa_download_debug is
 * refused (the per-point arrays are being rewritten). */
int lsa_extract_prefetch(lsa_ctx* ctx, int slot, const lsa_extract_params_t* params);
/* how many look-aheads lsa_extract_keypoints has adopted so far on this context */
int lsa_extract_prefetch_adopted(const lsa_ctx* ctx);
/* Keypoint types lsa_extract_keypoints keeps (bit k = type k; Slam::UseKeypoints, Slam.h:406): the others
 * come out empty, exactly as Slam::ExtractKeypoints drops them (Slam.cxx:789-793).  Default: all three. */
int lsa_set_keypoint_types(lsa_ctx* ctx, unsigned type_mask);

/* Copies a device keypoint set to the host.  Returns the number of points
 * written (<= capacity) or a negative error. */
int lsa_download_keypoints(lsa_ctx* ctx, int set, int type, lsa_point_t* out, int capacity);
int lsa_keypoint_count(const lsa_ctx* ctx, int set, int type);

/* SpinningSensorKeypointExtractor::GetDebugArray() (SSKE.cxx:640-680), one
 * array per call, in scan order.  array_id: 0 sin_angle, 1 saliency,
 * 2 depth_gap, 3 intensity_gap, 4/5/6 edge/plane/blob_keypoint,
 * 7/8/9 edge/plane/blob_validity. */
int lsa_download_debug(lsa_ctx* ctx, int array_id, float* out, int capacity);
int lsa_nb_laser_rings(const lsa_ctx* ctx);

/* Rigidly transforms a raw-current keypoint set in place (LIDAR -> BASE,
 * Slam::AggregateFrames(..., false), Slam.cxx:1551-1573) and adds time_offset
 * to every point's time. T is a row-major 4x4. */
int lsa_transform_keypoints(lsa_ctx* ctx, int set, int type, const double T[16], double time_offset);

/* ------------------------------------------------------------------------- */
/* Seam 2: KeypointsMatcher::BuildMatchResiduals(currPoints, kdtree, type)
 * -- slam_lib/src/KeypointsMatcher.cxx:33-74; the kd-tree build it replaces is
 *    KDTreePCLAdaptor::Reset, slam_lib/include/LidarSlam/KDTreePCLAdaptor.h:57-65. */

/* The reference keeps two independent families of kd-trees alive at the same time: the sub-map
 * trees of the rolling grids (rebuilt only on keyframes, RollingGrid.cxx:441) and the trees on the
 * previous scan's keypoints that ComputeEgoMotion builds every frame (Slam.cxx:845-860).  A target
 * therefore lives in a slot: */
#define LSA_TARGET_MAP 0       /* RollingGrid::GetSubMapKdTree() */
#define LSA_TARGET_PREVIOUS 1  /* kdtreePrevious of Slam::ComputeEgoMotion */

/* Sets the kNN target of one keypoint type from host points (the sub-map the
 * host-side RollingGrid produced, Slam.cxx:1003-1037) and builds the device
 * search grid.  Point order is kept: indices seen by the PCA are these. */
int lsa_set_target(lsa_ctx* ctx, int slot, int type, const lsa_point_t* pts, int m);
/* Same, from a device-resident keypoint set (ego-motion registers on the
 * previous frame's raw keypoints, Slam.cxx:845-860): no PCIe traffic. */
/* lsa_set_target without the wait: the caller fills a pinned host buffer owned by the context
 * (lsa_target_staging returns it, grown to `capacity` points; it may be called and filled from another host
 * thread, e.g. the one that extracts the sub-map) and lsa_set_target_staged enqueues the copy of its first m
 * points.  The buffer must stay untouched until the next match of that target has been waited for. */
lsa_point_t* lsa_target_staging(lsa_ctx* ctx, int slot, int type, int capacity);
int lsa_set_target_staged(lsa_ctx* ctx, int slot, int type, int m);
/* Ahead of its use: the staging buffer of (LSA_TARGET_MAP, type) holds m points that will probably become the target
 * (a sub-map extracted for the predicted pose).  They are uploaded and their search grid is built on the look-ahead
 * stream into a spare target; lsa_set_target_staged with the same m and cell size then only swaps it in.  Before the
 * staging buffer is rewritten instead (the prediction did not hold), lsa_drop_target_ahead waits for the copy out of
 * it.  lsa_staged_targets_adopted counts the take-overs. */
int lsa_stage_target_ahead(lsa_ctx* ctx, int slot, int type, int m);
int lsa_drop_target_ahead(lsa_ctx* ctx, int slot, int type);
int lsa_staged_targets_adopted(const lsa_ctx* ctx);
int lsa_set_target_from_set(lsa_ctx* ctx, int slot, int type, int set);
/* Builds ahead of time the targets the NEXT frame's ego-motion will search: the current raw keypoints of the types
 * in type_mask (which the next lsa_extract_keypoints turns into the previous ones) are copied and their search
 * grids built on the look-ahead stream, beside the current frame's registration.  The next
 * lsa_set_target_from_set(LSA_TARGET_PREVIOUS, type, LSA_SET_RAW_PREVIOUS) takes them over if the set was not
 * written since and the cell size is the one they were built with; otherwise it builds as usual.  Same neighbours
 * either way.  lsa_prepared_targets_adopted counts the take-overs. */
int lsa_prepare_previous_targets(lsa_ctx* ctx, unsigned type_mask);
int lsa_prepared_targets_adopted(const lsa_ctx* ctx);
int lsa_target_size(const lsa_ctx* ctx, int slot, int type);
/* The target's points as they were given (Slam::GetTargetSubMap, Slam.h:168): returns the number written. */
int lsa_download_target(lsa_ctx* ctx, int slot, int type, lsa_point_t* out, int capacity);
/* Edge length [m] of the search-grid cells used by the next lsa_set_target* of this type
 * (default 1.0; it is enlarged automatically when the grid would exceed 2^21 cells). */
int lsa_set_target_cell_size(lsa_ctx* ctx, int slot, int type, float cell);
/* Tuning only (results do not depend on it): lanes of a wavefront that cooperate on one query of `type`
 * in the first kNN kernel: 8, 16 or 32 (sparse targets such as edges: more lanes). */
int lsa_set_knn_lanes(lsa_ctx* ctx, int type, int lanes);
/* ... and the number of rounds of that kernel (2: blocks of 3^3 and 5^3 cells; 3: also 7^3) before a query is
 * handed to the second kernel. */
int lsa_set_knn_rounds(lsa_ctx* ctx, int type, int rounds);

/* MatchingResults::NbMatches() and the rejection histogram of an earlier match
 * (KeypointsMatcher.h:100-122) without reading anything back on the frame's
 * critical path: lsa_match_serial names the last match enqueued for a type, and
 * lsa_match_histogram reads that match's histogram later (it waits for the stream).
 * The device keeps the last 16 matches of every type. */
long long lsa_match_serial(const lsa_ctx* ctx, int type);
int lsa_match_histogram(lsa_ctx* ctx, int type, long long serial, int histogram[LSA_MATCH_NSTATUS]);
/* lsa_undistort(H0, H1, t0, t1) followed by lsa_match_types on LSA_SET_WORKING -- what comes between two iterations of
 * the localization ICP (Slam.cxx:1140-1147, 1074-1091) -- with the undistortion inside the search kernel when that kernel
 * reaches every keypoint of the working set (one-launch form, every type that has keypoints asked for, with a target and
 * valid parameters); as the two calls otherwise.  Same keypoints, same matches either way. */
int lsa_match_types_undistorted(lsa_ctx* ctx, int slot, unsigned type_mask, const lsa_match_params_t* p, const double pose[16], int* histograms,
                                const double H0[16], const double H1[16], double t0, double t1);
/* lsa_match_types as ONE launch for all keypoint types, search and model fit in the same kernel (on = 1, the default),
 * as two launches (on = 2: the searches of all types, then their model fits), or (on = 0) as the staged kernels, types
 * side by side on streams.  Same results either way. */
int lsa_set_fused_match(lsa_ctx* ctx, int on);
/* Diagnostics: queries of the last lsa_match that the first kNN kernel handed to the second stage. */
int lsa_match_slow_queries(lsa_ctx* ctx);
/* Diagnostics of the last fused match of `type` (LSA_ROUTE_STATS=1 when the context is created): [0] queries handed
 * to the tail kernel, [1] of them done, [2] second scans, [3] first block beyond shell 2, [4] candidates walked,
 * [5] NEIGHBORS_TOO_FAR by the counts, [6] first block = 3^3 finest cells, [7] longest walk of one lane. */
int lsa_match_route_stats(lsa_ctx* ctx, int type, int out[8]);
/* Diagnostics (LSA_ROUTE_STATS=1): {start, search end, model end, XCC | HW_ID} of the hardware blocks of the last
 * fused match, 100 MHz ticks. */
int lsa_match_trace(lsa_ctx* ctx, unsigned long long* out, int blocks);
/* ... and those of them that ended up scanning the whole target. */
int lsa_match_exhaustive_queries(lsa_ctx* ctx);

/* Replaces a device keypoint set by host points (used by tests and by callers
 * that aggregate several LiDAR devices on the host). */
int lsa_set_keypoints(lsa_ctx* ctx, int set, int type, const lsa_point_t* pts, int k);

/* For every keypoint of `type` in `query_set`: world = pose * X, exact kNN in
 * the target, neighbourhood filtering, PCA model fit, validity tests, residual
 * record (A, P, X, weight).  Records stay on the device for lsa_accumulate.
 * pose = PosePrior, row-major 4x4.  histogram[s] = number of keypoints with
 * MatchStatus s (MatchingResults::RejectionsHistogram). */
int lsa_match(lsa_ctx* ctx, int slot, int type, int query_set, const lsa_match_params_t* params, const double pose[16],
              int histogram[LSA_MATCH_NSTATUS]);

/* One ICP iteration's matching step (the `for (auto k : KeypointTypes)` loops of
 * Slam.cxx:895-912 and 1074-1091): every type in type_mask (bit k = type k) is
 * matched as by lsa_match, the types running concurrently on the device.
 * histograms: NULL, or [3][LSA_MATCH_NSTATUS] (rows of types outside the mask
 * are zero).  With NULL the call only enqueues work and returns without waiting
 * for the device; lsa_accumulate's n_valid then reports the number of matches. */
int lsa_match_types(lsa_ctx* ctx, int slot, unsigned type_mask, int query_set, const lsa_match_params_t* params, const double pose[16],
                    int* histograms);

/* Confidence::LCPEstimator (slam_lib/src/ConfidenceEstimators.cxx:27-65) as Slam::EstimateOverlap calls it
 * (Slam.cxx:1370-1388): every (1 / sampling_ratio)-th point of the current frame is registered into the
 * world (H0, or the H0 -> H1 interpolation of lsa_transform_frame when interpolate != 0), its nearest
 * neighbour is searched in the map-slot target of every type in type_mask that holds points, and the best
 * Gaussian score exp(-d^2 / (2 (leaf / 3)^2)) is averaged.  *overlap = -1 when nothing can be estimated.
 * The reference sums in float under an OpenMP reduction, i.e. in no defined order; agreement is to rounding. */
int lsa_overlap(lsa_ctx* ctx, unsigned type_mask, int interpolate, const double H0[16], const double H1[16], double t0, double t1, float sampling_ratio,
                const double leaf_size[3], float* overlap);

/* MatchingResults::Rejections / Weights of the last lsa_match of `type`
 * (exported by Slam::GetDebugArray, Slam.cxx:635-657).  records (optional,
 * may be NULL) receives 16 doubles per keypoint: A[9] row-major, P[3], X[3],
 * weight; rows of unmatched keypoints are zero. */
int lsa_download_match(lsa_ctx* ctx, int type, uint8_t* status, double* weights, double* records, int capacity);
/* Test hook: writes the match buffer of `type` as lsa_match would leave it -- n rows of the layout lsa_download_match
 * reads (A[9] row-major, P[3], X[3], weight), their status and the Tukey saturation distance -- so that lsa_accumulate
 * and the solves run on given residual blocks.  Rows whose status is not LSA_MATCH_SUCCESS are stored as given (any
 * payload, NaN included): the reductions never read them into a sum.  The buffer grows as lsa_match grows it. */
int lsa_upload_match(lsa_ctx* ctx, int type, const uint8_t* status, const double* records, int n, double saturation);
#define LSA_KNN_MAX 16 /* slots per query of the neighbour lists (the search holds at most 16 neighbours) */
/* Test hook: the neighbour lists the last search of `type` left in memory -- the two-launch form (lsa_set_fused_match 2),
 * the staged form (0) and lsa_overlap's nearest-neighbour search leave them; the one-launch form (1) keeps them on the
 * chip, and 0 is returned after it.  For the first n = min(capacity, queries) queries, one row of LSA_KNN_MAX slots per
 * query: idx[q * LSA_KNN_MAX + s] is the index in the target (the order it was given in) of the (s + 1)-th nearest
 * point, d2[q * LSA_KNN_MAX + s] the float squared distance the search compared, ascending by (distance, index).  A slot
 * at or beyond the number of neighbours found holds (INT32_MAX, +inf) where the search asked for it and (-1, +inf)
 * beyond the k it asked for.  cnt[q] as stored:
 *   >= 0  the number of neighbours found, min(k, target size);
 *   -1    planes and blobs only: the k-th neighbour is proven to lie beyond the rejection distance
 *         (NEIGHBORS_TOO_FAR whatever the neighbours are) -- the slots need not hold the nearest points;
 *   -2    two-launch form only: no block of the grid settled the query, the model kernel searched the whole target for
 *         it and wrote the answer into the slots -- the count stays as the search kernel left it.
 * Returns n.  Host code and copies only. */
int lsa_download_knn(lsa_ctx* ctx, int type, int* idx, float* d2, int* cnt, int capacity);

/* ------------------------------------------------------------------------- */
/* Seam 3: LocalOptimizer::Solve() -- slam_lib/src/LocalOptimizer.cxx:74-102.
 * The device evaluates what Ceres evaluates per LM step for the residual
 * blocks of the last lsa_match calls of the types in type_mask (bit k = type
 * k), in the order EDGE, PLANE, BLOB (Slam.cxx:936-937, 1120-1121):
 *   r_i = A_i (R(rpy) X_i + t - P_i),  rho = weight_i * Tukey(|r_i|^2)
 *   cost = 1/2 sum rho,  g = sum rho' J^T r,  H = sum rho' J^T J (upper part
 *   mirrored, row-major 6x6), w = (x, y, z, rx, ry, rz).
 * The 6-dof trust-region control flow itself stays on the host (it is a
 * 6x6 solve); see lidarslam_amd/csrc/host/lsa_lm_loop.cpp. */
int lsa_accumulate(lsa_ctx* ctx, unsigned type_mask, const double w[6], int want_jacobian, double* cost, double g[6],
                   double H[36], int* n_valid);
/* 1 when the partial sums of lsa_accumulate arrive through coherent host memory the kernel writes directly (the
 * normal case), 0 when that memory could not be mapped and every evaluation falls back to a copy + synchronise
 * (same results, about twice the time per evaluation). */
int lsa_mailbox_active(const lsa_ctx* ctx);

/* LocalOptimizer::SetPosePrior + Solve + GetOptimizedPose (LocalOptimizer.cxx:44-48, 74-109) on the
 * device-resident residual blocks of type_mask: the Ceres trust-region Levenberg-Marquardt loop
 * (DENSE_QR, max_num_iterations = lm_max_iter, TwoDMode holds Z, rX, rY) with every evaluation on
 * the GPU.  summary[0] = num_successful_steps (counts iteration 0, as ceres::Solver::Summary does:
 * == 1 means no step was accepted, Slam.cxx:950), [1] unsuccessful steps, [2] iterations,
 * [3] evaluations; costs[0] initial, [1] final. */
int lsa_solve(lsa_ctx* ctx, unsigned type_mask, const double prior[16], int lm_max_iter, int two_d_mode, double optimized[16],
              int summary[4], double costs[2]);
/* The same solve as ONE launch: the trust-region loop itself runs on the device (every block evaluates its share
 * of the residual blocks, the blocks exchange their partial sums through tagged 8-byte granules, each block runs the
 * 6x6 algebra), the host only reads the result.  prior / pose are the six parameters (x, y, z, rx, ry, rz) of
 * LocalOptimizer::PoseArray (LocalOptimizer.h:99-101).  min_matches: Slam.cxx:919, 1098 skip the optimisation when
 * fewer keypoints matched (skipped = 1, pose = prior).  cost, g, H: the normal equations at the returned pose (what
 * EstimateRegistrationError needs).  Returns LSA_E_STATE when the device gave up (blocks not co-resident in time):
 * the caller then runs lsa_solve / the host-driven loop; nothing was changed. */
typedef struct lsa_solve_result
{
  double pose[6];
  double initial_cost, final_cost;
  double cost, g[6], H[36];
  int num_successful_steps;   /* counts iteration 0, as ceres::Solver::Summary does */
  int num_unsuccessful_steps;
  int num_iterations;
  int num_evaluations;
  int num_matches;            /* residual blocks (successful matches) the problem was built from */
  int skipped;
  int termination;            /* 0 none, 1 not enough matches, 2 gradient tolerance at iteration 0, 3 max iterations,
                                 4 gradient tolerance, 5 min trust region radius, 6 too many invalid steps,
                                 7 parameter tolerance, 8 function tolerance */
  const char* message;
} lsa_solve_result_t;
int lsa_solve_device(lsa_ctx* ctx, unsigned type_mask, const double prior[6], int two_d_mode, int lm_max_iter, int min_matches,
                     lsa_solve_result_t* out);
/* lsa_solve_device in two halves: _begin enqueues the solve (prior == NULL: the start point is the one the link in
 * front of it will hold, see lsa_icp_link), _end waits for the result of the oldest solve begun and not ended.
 * _drop forgets the solve begun last without waiting (its link was called off: it will never run). */
int lsa_solve_device_begin(lsa_ctx* ctx, unsigned type_mask, const double prior[6], int two_d_mode, int lm_max_iter, int min_matches);
int lsa_solve_device_end(lsa_ctx* ctx, lsa_solve_result_t* out);
int lsa_solve_device_drop(lsa_ctx* ctx);

/* ICP iterations enqueued AHEAD of their inputs (the `for icpIter` loops of Slam::ComputeEgoMotion / Localization,
 * slam_lib/src/Slam.cxx:892-950, 1071-1145: iteration i + 1 needs the pose iteration i ends with), without the host
 * between two iterations.  A LINK is a block of 64 words on the device that the solve in front of it fills in itself: word
 * 0 = go -- whether the next iteration runs (Slam.cxx:919-923, 950 / 1098-1107, 1151: the solve was not skipped and made
 * a step) -- then the pose from the solve's parameters (Utils::XYZRPYtoIsometry), the next start point
 * (LocalOptimizer::SetPosePrior's IsometryToXYZRPY of that pose) and, localization, the constants of
 * Slam::RefineUndistortion under the new pose (Slam.cxx:1322-1352) -- with the arithmetic the host uses on the same result
 * when it arrives (lsa_posemath.h over lsa_pmath.h: the same bits).  The launches enqueued behind a link -- a match with
 * lsa_match_types_linked, a solve with prior == NULL -- read their inputs from it ON THE DEVICE, or do nothing when go is
 * not 1.  A whole loop is enqueued at once:
 *   lsa_match_types(...)                                       iteration 0, pose from the host
 *   t1 = lsa_icp_link(ctx)                                     reserves a block (at most 7 at a time)
 *   lsa_solve_device_begin_linked(.., prior, .., t1, &link)    solve 0 leaves block t1; what is enqueued next waits behind it
 *   lsa_match_types_linked(...)                                 iteration 1: searches under the pose in t1, or does nothing
 *   t2 = lsa_icp_link(ctx); lsa_solve_device_begin_linked(.., NULL, .., t2, &link); ...
 *   lsa_solve_device_begin_linked(.., NULL, .., -1, NULL)      the last one leaves nothing
 * then lsa_solve_device_end once per iteration, in order; the host takes the same decision from every result and, where
 * the device stopped, forgets the rest with lsa_icp_abandon.  Between two iterations there is one kernel boundary.
 * lsa_icp_cancel(ctx, ticket) takes back what the match behind that link announced on the host (the device has called the
 * iteration off itself, or will never reach it); lsa_icp_abandon does so for every link still reserved, the youngest
 * first, and forgets the solves begun behind them (error paths, Reset).
 * lsa_match_types_linked returns 1 (and enqueues nothing) when this match cannot wait behind a link: the two-launch or
 * staged forms, an empty target, an undistortion that would not reach every keypoint. */
int lsa_icp_cancel(lsa_ctx* ctx, int ticket);
int lsa_icp_abandon(lsa_ctx* ctx);
int lsa_match_types_linked(lsa_ctx* ctx, int slot, unsigned type_mask, int query_set, const lsa_match_params_t* p, int undistort);
typedef struct lsa_icp_link
{
  int refine_undistortion;         /* localization: Slam::RefineUndistortion between two iterations (Undistortion = REFINED) */
  int first;                       /* first solve of the loop: the motion within the frame is `motion` (later solves go on
                                      from what the solve before them left on the device) */
  int have_log;                    /* Slam::InterpolateScanPose (Slam.cxx:1271-1285): LogTrajectory is not empty, */
  double prev_time, cur_time;      /*   its last time and the current frame's [s], */
  double max_extrapolation_ratio;  /*   MaxExtrapolationRatio */
  double previous_world[16];       /* PreviousTworld */
  double motion[16];               /* LinearTransformInterpolator: Time0, Time1, Rot0 (w x y z), Rot1, Trans0[3], Trans1[3] */
} lsa_icp_link_t;
int lsa_icp_link(lsa_ctx* ctx);
int lsa_solve_device_begin_linked(lsa_ctx* ctx, unsigned type_mask, const double prior[6], int two_d_mode, int lm_max_iter, int min_matches,
                                  int leave_ticket, const lsa_icp_link_t* link);
/* Test hook: the block of `ticket` as the device holds it now (waits for the context's stream): words[0] = go, then pose
 * R[9] t[3], start point [6], and the undistortion's constants (64 words in all, doubles unless stated in lsa_posemath.h). */
int lsa_icp_link_peek(lsa_ctx* ctx, int ticket, unsigned long long words[64]);
/* ... and the block the HOST's arithmetic gives for a solve that ended at `x` (its result's skipped / successful steps decide
 * whether the next iteration runs): what lsa_icp_link_peek must show, word for word wherever go == 1 (with go == 0 only
 * word 0 counts).  motion_after (may be NULL): the LinearTransformInterpolator state after the refinement. */
int lsa_icp_link_expected(const double x[6], int skipped, int successful_steps, const lsa_icp_link_t* link, unsigned long long words[64], double motion_after[16]);

/* Diagnostics (LSA_ROUTE_STATS=1): 100 MHz ticks block 0 spent evaluating, exchanging, folding, stepping, summed over
 * the solves so far; [4] evaluations, [5] ticks inside the kernel, [6] solves, [7] of evaluating: the residual blocks alone,
 * [8..11] of stepping: decision, scaled system, Cholesky solve, model change and candidate.  All 12 slots keep their
 * meaning from build to build; a part a later kernel no longer has reads 0.  As k_lm_solve stands: "exchanging" ends when
 * thread 0 holds its own granules of every workgroup, "folding" is its sums, the 8-lane addition, the one barrier behind them
 * and the sensor terms; "stepping" no longer holds the rotation derivatives of a point past the end of the solve. */
int lsa_solve_device_trace(lsa_ctx* ctx, unsigned long long out[12]);
/* Test hook for the bounded wait on the device, so that the callers' fall-back can be exercised:
 *   "lm_give_up_block" b     workgroup b of the NEXT one-launch solve abandons the exchange (the others then wait their
 *                            20 ms and give up too: lsa_solve_device reports LSA_E_STATE); one shot, -1 = none
 * and the launch shapes of the two reductions, as the environment sets them at creation, with the same clamps; a
 * negative value restores what the context was created with; they take effect at the next launch:
 *   "lm_blocks" (LSA_LM_BLOCKS 1..128), "lm_records" (LSA_LM_RECORDS 256..4096), "lm_cache" (LSA_LM_CACHE, at most the
 *   LDS layers the solve kernel has room for), "accum_blocks" (LSA_ACCUM_BLOCKS 1..256), "mailbox_check" (LSA_MAILBOX_CHECK)
 * and of the keypoint log: "kplog_chunk_kib" n (chunks made from now on hold n KiB; negative: 32 MiB again), "kplog_fail_alloc"
 * 1 / 0 (while 1, a chunk allocation fails as if the device were out of memory);
 * and of the map descriptors: "map_describe_slice" n (points a slice of the next description; <= 0: 4096), "map_describe_cull"
 * 1 / 0 (slices out of a viewpoint's reach are passed over, or read like the others: the same bytes either way) */
int lsa_debug_set(lsa_ctx* ctx, const char* name, int value);
/* The shape of the last one-launch solve (lsa_solve_device_begin): {workgroups, residual blocks per thread, of those kept
 * in LDS, residual blocks in all}. */
int lsa_solve_device_shape(const lsa_ctx* ctx, int out[4]);
/* The shape of the last lsa_accumulate: {workgroups, most residual blocks of one thread, 0, residual blocks in all}. */
int lsa_accumulate_shape(const lsa_ctx* ctx, int out[4]);
/* Solves the device gave up on so far (diagnostics; 0 on a healthy run). */
int lsa_solve_device_fallbacks(const lsa_ctx* ctx);
/* Host work for the time the next solve runs on the device: `fn(arg)` is called once, on the calling thread, by the
 * next lsa_solve_device after it has enqueued its kernel and before it waits for the result (enqueueing work that does
 * not depend on the solve, e.g. on another stream).  NULL withdraws it. */
int lsa_solve_device_interlude(lsa_ctx* ctx, void (*fn)(void*), void* arg);
/* LocalOptimizer::EstimateRegistrationError (LocalOptimizer.cxx:112-140) at `pose`: covariance
 * (row-major 6x6, DoF order X,Y,Z,rX,rY,rZ), err[0] position error [m], err[1] orientation error [deg]. */
int lsa_registration_error(lsa_ctx* ctx, unsigned type_mask, const double pose[16], int two_d_mode, double cov[36], double err[2]);

/* ------------------------------------------------------------------------- */
/* External sensor constraints of the localization problem (Slam.cxx:1123-1131, CeresCostFunctions.h:255-341).
 * Both act on the world pose w = (X, Y, Z, rX, rY, rZ) under ScaledLoss(NULL, weight):
 *   wheel    r = |t - p| - d           (|t - p| replaced by 0, and its Jacobian by 0, where |t - p|^2 < 1e-6)
 *   gravity  r = R(rX, rY, rZ) g_cur - g_ref
 * cost += 1/2 weight |r|^2, g += weight J^T r, H += weight J^T J; the match count is not touched. */
typedef struct lsa_sensor_terms_t
{
  int wheel;          /* 1: the odometer term is in the problem */
  double wheel_weight;
  double p[3];        /* origin the travelled distance is measured from (the reference's PreviousPose: identity) */
  double d;           /* distance travelled since the first frame with a measurement */
  int gravity;        /* 1: the gravity alignment term is in the problem */
  double gravity_weight;
  double g_ref[3];    /* reference gravity direction (unit) */
  double g_cur[3];    /* gravity direction measured at the frame's time (unit) */
} lsa_sensor_terms_t;
/* The terms enter every lsa_accumulate, lsa_solve, lsa_solve_device(_begin / _linked) and lsa_registration_error of the
 * context from now on (a solve enqueued ahead carries the terms of the moment it was enqueued); NULL clears them. */
int lsa_set_sensor_terms(lsa_ctx* ctx, const lsa_sensor_terms_t* terms);
/* Host evaluation of the terms at w (rotation from libm sin / cos): sums[29] = cost, g[6], H upper triangle row by row
 * (21), count -- the layout of the device's normal equations; sums are overwritten, not added to. */
int lsa_sensor_terms_eval(const lsa_sensor_terms_t* terms, const double w[6], double sums[29]);

/* The reference's measurement managers (SensorConstraints.h / .cxx: WheelOdometryManager absolute mode, ImuManager) on
 * the host, without a device: what Slam::ComputeSensorConstraints makes of the measurements at one LiDAR time.
 * lsa_sensors_compute applies the whole rule of Slam::AddFrames: when neither manager is usable (weight > 1e-6 and at
 * least one measurement) nothing is computed and the previous terms are returned again. */
typedef struct lsa_sensors lsa_sensors;
lsa_sensors* lsa_sensors_create(void);
void lsa_sensors_destroy(lsa_sensors* s);
int lsa_sensors_add_wheel_odom(lsa_sensors* s, double time, double distance);
int lsa_sensors_add_gravity(lsa_sensors* s, double time, const double acc[3]);
int lsa_sensors_set_weights(lsa_sensors* s, double wheel_weight, double gravity_weight);
int lsa_sensors_set_time_offset(lsa_sensors* s, double offset);
/* ClearSensorMeasurements: measurements and terms cleared, time offset 0; the gravity reference and the odometer
 * baseline are kept */
int lsa_sensors_clear(lsa_sensors* s);
int lsa_sensors_compute(lsa_sensors* s, double lidar_time, lsa_sensor_terms_t* out);
/* the gravity reference (zero until first needed); returns 1 when it has been computed */
int lsa_sensors_gravity_ref(const lsa_sensors* s, double g[3]);

/* ------------------------------------------------------------------------- */
/* Seam 4: undistortion / transforms.                                         */

/* CurrentUndistortedKeypoints = CurrentRawKeypoints (Slam.cxx:984). */
int lsa_reset_working_keypoints(lsa_ctx* ctx);

/* Slam::RefineUndistortion's per-point loop (Slam.cxx:1342-1351): every point
 * of every LSA_SET_WORKING type is transformed in place by the pose
 * interpolated at its `time` between H0 (at t0) and H1 (at t1)
 * (LinearTransformInterpolator::operator(), MotionModel.h:115-129).
 * H0/H1 row-major 4x4.  If t0 == t1 or H0 ~ H1 the interpolator is invalid and
 * H0 is applied to every point, as in the reference. */
int lsa_undistort(lsa_ctx* ctx, const double H0[16], const double H1[16], double t0, double t1);

/* What Slam::Localization starts with (Slam.cxx:980-999, 1026-1029) as ONE launch: lsa_reset_working_keypoints, then
 * lsa_undistort(H0, H1, t0, t1) unless H0 is NULL, then -- unless box_pose is NULL -- the bounding boxes of the three
 * types under box_pose as lsa_keypoint_bboxes_begin(LSA_SET_WORKING, box_pose) leaves them on the device for the
 * device maps (lsa_device_grid_build_submap_begin_for_keypoints, lsa_device_grid_submap_ahead_take); they only travel
 * to the host if lsa_keypoint_bboxes_end asks for them.  Same working keypoints and boxes as the separate calls.
 * lsa_arm_localization_boxes prepares the boxes' words for that launch (one tiny launch): called while the device is
 * idle -- between two frames -- it is off the frame's critical path; lsa_localization_begin does it itself otherwise. */
int lsa_localization_begin(lsa_ctx* ctx, const double H0[16], const double H1[16], double t0, double t1, const double box_pose[16]);
int lsa_arm_localization_boxes(lsa_ctx* ctx);

/* min/max of the `time` field over the working keypoints (Slam::InitUndistortion,
 * Slam.cxx:1291-1300) and bounding box of pose * working keypoints of one type
 * (Slam.cxx:1026-1029). */
int lsa_working_time_range(lsa_ctx* ctx, double* tmin, double* tmax);
/* ... of any keypoint set (the raw sets get theirs from the extraction at no cost) */
int lsa_keypoint_time_range(lsa_ctx* ctx, int set, double* tmin, double* tmax);
int lsa_working_bbox(lsa_ctx* ctx, int type, const double pose[16], float mn[3], float mx[3]);
/* The same for the three keypoint types in one pass and one synchronisation:
 * mn / mx = [type][xyz]. */
int lsa_working_bboxes(lsa_ctx* ctx, const double pose[16], float mn[9], float mx[9]);
/* The same on any keypoint set, split in two: _begin only enqueues the reduction and its read-back, _end
 * waits for exactly that work.  Whatever the caller enqueues in between overlaps it. */
int lsa_keypoint_bboxes_begin(lsa_ctx* ctx, int set, const double pose[16]);
/* Same with the pose interpolated at every point's own time between H0 (at t0) and H1 (at t1), like lsa_undistort:
 * the box the keypoints will have once they are undistorted with that motion. */
int lsa_keypoint_bboxes_begin_interp(lsa_ctx* ctx, int set, const double H0[16], const double H1[16], double t0, double t1);
int lsa_keypoint_bboxes_end(lsa_ctx* ctx, float mn[9], float mx[9]);
/* The boxes of a prediction, for lsa_device_grid_submap_ahead_begin only: as lsa_keypoint_bboxes_begin(_interp when H1 is
 * given) but enqueued on the context's look-ahead stream (where the device maps work) and never copied to the host, so that
 * nothing of the speculation sits on the context's own stream.  _mark, called by the thread that drives the context once
 * the set's keypoints are enqueued, names the point from which they exist; lsa_keypoint_boxes_predicted may then be
 * called from any thread. */
int lsa_keypoint_boxes_predicted_mark(lsa_ctx* ctx);
int lsa_keypoint_boxes_predicted(lsa_ctx* ctx, int set, const double H0[16], const double H1[16], double t0, double t1);

/* Slam::TransformPointCloud (Slam.cxx:1491-1509) on a device keypoint set:
 * writes pose * set to `out` on the host. */
int lsa_download_transformed(lsa_ctx* ctx, int set, int type, const double pose[16], lsa_point_t* out, int capacity);
/* The same for the three types of a set at once and without waiting: the device writes the transformed
 * points straight into pinned host buffers owned by the context.  lsa_staged_transformed waits for that
 * work only (it may be called from another host thread, e.g. the one that inserts the points into a map)
 * and returns the buffer of one type; it stays valid until the next lsa_stage_transformed. */
int lsa_stage_transformed(lsa_ctx* ctx, int set, const double pose[16]);
int lsa_staged_transformed(lsa_ctx* ctx, int type, const lsa_point_t** pts, int* n);

/* Slam::AggregateFrames(frames, true) (Slam.cxx:1512-1578): the whole current
 * frame to WORLD.  interpolate != 0: per-point pose between H0 (t0) and H1
 * (t1); else rigid H0. */
int lsa_transform_frame(lsa_ctx* ctx, int interpolate, const double H0[16], const double H1[16], double t0, double t1,
                        lsa_point_t* out, int capacity);
/* Same for a further frame of a multi-device AddFrames call: every point's time is shifted by time_offset first
 * (frame stamp - first frame's stamp, Slam.cxx:1536-1549) and stored shifted. */
int lsa_transform_frame_at(lsa_ctx* ctx, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset,
                           lsa_point_t* out, int capacity);

/* Device self-test of the arithmetic the bit-exact parity rests on: evaluates fn on the GPU for n
 * inputs.  fn: 0 lsa_sin(x) 1 lsa_cos(x) 2 lsa_atan2(y, x) 3 (float)sqrt((float)x)
 * 4 (float)x / (float)y  5 sqrt(x)  6 x / y.  Results as doubles. */
int lsa_selftest_math(lsa_ctx* ctx, int fn, const double* x, const double* y, int n, double* out);
/* Device self-test of the fixed-size solvers the kernels inline, evaluated by the same templates: n records of
 * doubles, one thread per record, record i at in + i * IN and out + i * OUT.  Points are rounded to float, Sym3 and
 * eigen33 of fn 0 and 2 work in float; Sym3 = xx xy xz yy yz zz; e0 e1 e2 = eigenvectors of l0 <= l1 <= l2; pose
 * matrices are R row-major (9) then t (3); quaternions w x y z.
 *   fn  IN  OUT
 *    0  49  15  PCA_F   CovAccum<float> + eigen33<float>. in: k (1..16), k points x y z (48 slots).
 *                       out: mean[3] l0 l1 l2 e0[3] e1[3] e2[3]
 *    1  49  15  PCA_D   the same with CovAccum<double> + eigen33<double> (float points)
 *    2   6  12  EIG33_F eigen33<float> of a Sym3. out: l0 l1 l2 e0[3] e1[3] e2[3]
 *    3   6  12  EIG33_D eigen33<double>
 *    4  12   4  SPD3    solve_spd<3>. in: A[9] row-major, b[3]. out: ok (1/0), x[3] (0 where not reached)
 *    5  42   7  SPD6    solve_spd<6>. in: A[36], b[6]. out: ok, x[6]
 *    6  23  28  ACCUM   rotation_and_derivatives + accumulate_one of one residual block at pose w.
 *                       in: A[9] P[3] X[3] weight sat w[6] (x y z rx ry rz; Tukey a^2 = sat * sat).
 *                       out: cost, g[6], H upper triangle row-major[21]
 *    7  42  39  POSE    in: M0[12] M1[12] w[6] qa[4] qb[4] s t t0 t1.  out: FromXYZRPY(w)[12], ToXYZRPY(M0)[6],
 *                       ToQuaternion(M0)[4], Slerp(qa, qb, s)[4], RotationAngle(M0), interp_eval of
 *                       MakeInterpConst(M0, M1, t0, t1) at t [12]
 *    8  12   4  SPD3_HOST   SolveSPD of the host LM loop (host/lsa_lm_loop.cpp), layout of fn 4
 *    9  42   7  SPD6_HOST   layout of fn 5
 *   10   9  12  JACOBI3_HOST  the host's cyclic Jacobi eigen-solver. in: A[9]. out: evals[3] ascending, V[9] row-major
 *                            (columns = eigenvectors)
 *   11  36  42  JACOBI6_HOST  in: A[36]. out: evals[6], V[36]
 * fn 8-11 run on the CPU and accept ctx == NULL. */
int lsa_selftest_numerics(lsa_ctx* ctx, int fn, const double* in, int n, double* out);
/* Self-test of the trust-region step of the LM solve on scripted sums: what the solve does between two evaluations --
 * step acceptance, radius update, damped Cholesky solve, the invalid-step retry, the ways of ending -- reads 29 sums per
 * evaluation, its own state, max_iter and min_matches, and nothing of the residual blocks.  lsa_selftest_lm_step runs the
 * device's step (lm_step of lsa_lm.hip, the code lsa_solve_device inlines) with one workgroup per script, all scripts in
 * one launch; lsa_selftest_lm_host runs the host loop (host/lsa_lm_loop.cpp, the code behind lsa_solve) and needs neither
 * a context nor a device.  Same arguments, same outputs, bit for bit.
 *   header[4 * s ..]  two_d, max_iter (>= 0), min_matches, K (1..4096) of script s
 *   x0[6 * s ..]      its start point x y z rx ry rz
 *   sums              the scripts' evaluations one after the other, script s's K first; an evaluation is 29 doubles:
 *                     cost, g[6], the upper triangle of H row by row [21], the number of residual blocks.  Evaluation 0
 *                     is the one at x0; evaluation k + 1 is taken for the candidate record k holds, wherever that is.
 *                     In 2D mode the rows and columns z rx ry of g and H are never read.
 *   records           one record of 42 doubles per evaluation, in the order of `sums` (all 0 behind the stop):
 *                       [0..5] the next candidate (0 when the solve is over)  [6] termination code  [7] 1: the solve is over
 *                       [8] radius  [9] decrease_factor  [10] |x| over the active parameters  [11] model_cost_change
 *                       [12] |step|  [13] initial_cost  [14] reuse_diagonal  [15] consecutive invalid steps  [16] iteration
 *                       [17] evaluations, the candidate's included  [18] successful  [19] unsuccessful steps  [20] iterations
 *                       [21] skipped  [22] matches  [23..28] the current point  [29..34] Jacobi scales and [35..40] LM
 *                       diagonal of the active parameters, in their order (1 and 0 behind them)
 *                       [41] parity of the evaluations whose sums became the current ones (the device's buffer index)
 *   results[45 * s ..] as lsa_solve_device_end receives it: pose[6], initial cost, final cost, the 29 sums at the final
 *                     point, successful, unsuccessful, iterations, evaluations, skipped, termination, matches, 0
 *   status[2 * s ..]  0: the solve ended / 1: the script ran out first (records up to there, result all 0); evaluations used
 * The number of residual blocks of an evaluation must be finite.  Returns LSA_E_ARG for a bad header. */
int lsa_selftest_lm_step(lsa_ctx* ctx, int n_scripts, const int* header, const double* x0, const double* sums, double* records, double* results, int* status);
int lsa_selftest_lm_host(int n_scripts, const int* header, const double* x0, const double* sums, double* records, double* results, int* status);
/* Device self-test of the keypoint labelling (SetKeyPointsLabels, SSKE.cxx:474-590) on its own: the labelling kernel of
 * the extraction, launched as the extraction launches it, on scores and validity the caller provides instead of those
 * the curvature kernels computed.  nrings (1..512) rings of ring_lengths[r] >= 0 points; the four score arrays and
 * `valid` (bit k = valid for keypoint type k) hold the rings one after the other.  Scores are what the curvature
 * kernel can produce: non-negative, finite or +inf, no -0.0, no NaN.  Of params, neighbor_width and the five
 * thresholds are used.  label_out / valid_out: one byte per point (bit k = type k; validity after the labelling, the
 * bit of a labelled point set back as SSKE.cxx:584 does); ring_counts_out[3 * r + k] = keypoints of type k on ring r.
 * Returns the number of points, LSA_E_CAPACITY when a ring has more than 8192 points (as the extraction does).  The
 * per-point arrays of the last extraction (lsa_download_debug) are overwritten; the keypoint sets are not touched. */
int lsa_selftest_labels(lsa_ctx* ctx, const lsa_extract_params_t* params, const int* ring_lengths, int nrings, const float* sin_angle,
                        const float* depth_gap, const float* saliency, const float* intensity_gap, const uint8_t* valid,
                        uint8_t* label_out, uint8_t* valid_out, int* ring_counts_out);
/* Diagnostic: `blocks` single-wave workgroups sleep-spinning for `ms` (<= 2000) milliseconds on a side stream. */
int lsa_selftest_keep_busy(lsa_ctx* ctx, int ms, int blocks);

/* ------------------------------------------------------------------------- */
/* Per-kernel timing of the last call sequence (HIP events on the context's   */
/* stream), for bench.py's roofline block.                                    */
typedef struct lsa_kernel_stat_t
{
  char name[48];
  uint32_t launches;
  double total_ms;
  double bytes;   /* algorithmic bytes summed over the launches */
} lsa_kernel_stat_t;
int lsa_profile_enable(lsa_ctx* ctx, int on);
/* What a pair of HIP events measures around nothing on the context's stream [us] (calibrated when profiling is switched
 * on; every scope's time is what its events measure minus this). */
double lsa_profile_event_overhead_us(const lsa_ctx* ctx);
/* Events cost a few microseconds per scope on a path that is launch bound: time only the scope `scope`,
 * and only one launch in `every` of it (all launches are counted; total_ms is scaled to all of them). */
int lsa_profile_select(lsa_ctx* ctx, const char* scope, int every);
int lsa_profile_reset(lsa_ctx* ctx);
int lsa_profile_get(lsa_ctx* ctx, lsa_kernel_stat_t* out, int capacity);

/* ------------------------------------------------------------------------- */
/* Pipeline level: LidarSlam::Slam behind a C handle (what a ctypes / cgo /
 * JNI user binds).  Mirrors Slam::AddFrame / GetWorldTransform
 * -- slam_lib/include/LidarSlam/Slam.h:111-146.                              */
typedef struct lsa_slam lsa_slam;

int lsa_slam_create(int device_id, lsa_slam** out);
void lsa_slam_destroy(lsa_slam* s);
const char* lsa_slam_last_error(const lsa_slam* s);
/* Generic parameter access by the reference's setter name without "Set",
 * e.g. "EgoMotion", "Undistortion", "LocalizationICPMaxIter", "NbThreads",
 * "VoxelGridLeafSizeEdges" ...  Returns LSA_E_ARG for an unknown name. */
int lsa_slam_set_param(lsa_slam* s, const char* name, double value);
int lsa_slam_get_param(const lsa_slam* s, const char* name, double* value);
void lsa_slam_reset(lsa_slam* s, int reset_log);
/* Slam::ClearMaps: empties the three keypoint maps; poses and parameters stay. */
int lsa_slam_clear_maps(lsa_slam* s);
/* Slam::AddFrame: frame = host scan, stamp_us = pcl header.stamp, seq = header.seq. */
int lsa_slam_add_frame(lsa_slam* s, const lsa_point_t* pts, int n, uint64_t stamp_us, uint32_t seq);
/* Same on a scan already resident in the frame store of the underlying context. */
int lsa_slam_store_frame(lsa_slam* s, int slot, const lsa_point_t* pts, int n);
int lsa_slam_add_stored_frame(lsa_slam* s, int slot, uint64_t stamp_us, uint32_t seq);
/* Replay from the frame store: names the slot of the frame that will be added after the next one, so that its
 * keypoints are extracted beside the registration of that frame (lsa_extract_prefetch).  Purely a scheduling hint:
 * the results are the same with or without it, and a hint that does not come true costs one wasted extraction. */
int lsa_slam_hint_next_stored_frame(lsa_slam* s, int slot);
/* The same for replay from HOST clouds: announces the cloud of the lsa_slam_add_frame call after the next one.  Its
 * upload starts at once and runs beside the registration of the frame in between (pinned staging, a copy stream and a
 * thread of its own: lsa_upload_frame_begin), its keypoints are extracted as soon as it has arrived; the
 * lsa_slam_add_frame that is handed this very buffer (same pointer, same size) takes both over.  The buffer must stay
 * valid and unchanged until that call returns.  Results are the same with or without the hint. */
int lsa_slam_hint_next_frame(lsa_slam* s, const lsa_point_t* pts, int n);
/* Slam::GetWorldTransform: row-major 4x4 + time [s]. */
int lsa_slam_get_world_transform(const lsa_slam* s, double T[16], double* time);
int lsa_slam_get_covariance(const lsa_slam* s, double cov[36]);
/* Slam::GetKeypoints(k, world): number of points written. */
int lsa_slam_get_keypoints(lsa_slam* s, int type, int world, lsa_point_t* out, int capacity);
/* Slam::GetRegisteredFrame. */
int lsa_slam_get_registered_frame(lsa_slam* s, lsa_point_t* out, int capacity);
/* Slam::GetDebugArray entries "EgoMotion: <type> matches" / "Localization: ...". */
int lsa_slam_get_match_status(lsa_slam* s, int localization, int type, uint8_t* status, double* weights, int capacity);
/* Slam::GetDebugInformation-like counters and stage timings [s]:
 * out[0] total, [1] extract, [2] ego_icp, [3] ego_lm, [4] loc_icp, [5] loc_lm,
 * [6] undistort, [7] submap, [8] maps, [9] ego_iters, [10] loc_iters,
 * [11] lm_evals, [12] total matched, [13] keyframe counter, [14] wait for the
 * previous keyframe's asynchronous map insertion, [15] duration of that insertion. */
int lsa_slam_get_stats(const lsa_slam* s, double out[16]);

/* The remaining result getters of Slam.h:141-189.
 * - GetLatencyCompensatedWorldTransform (Slam.cxx:555-590): the last pose extrapolated by the duration of the last
 *   AddFrame (parameter "Latency").
 * - SetWorldTransformFromGuess (Slam.cxx:490-501).
 * - GetTrajectory / GetCovariances (Slam.cxx:593-605): rows of 17 doubles (row-major 4x4 + time [s]) and of 36;
 *   either pointer may be NULL; returns the number of logged poses (parameter "LoggingTimeout": 0 keeps two).
 * - GetDebugInformation (Slam.cxx:610-633): [0..1] ego-motion edges / planes used, [2..4] localization edges /
 *   planes / blobs used, [5] position error, [6] orientation error, [7] overlap, [8] comply motion limits,
 *   [9] latency [s].
 * - GetMap(k, clean) / GetTargetSubMap(k) (Slam.cxx:670-688): return the full size, write at most capacity points. */
int lsa_slam_get_latency_compensated_world_transform(const lsa_slam* s, double T[16], double* time);
/* Several LiDAR devices on one platform (Slam.h:133-138, 239-250; Slam.cxx:753-801, 1512-1578).
 * - lsa_slam_add_frames = Slam::AddFrames: one frame per device (at most 16), each with its own stamp; the device is
 *   the device_id of the frame's first point; the pose is dated by the first frame's stamp.  Every frame is extracted
 *   with its device's extractor and the keypoints are merged in frame order, moved to BASE by the device's offset and
 *   shifted in time by (its stamp - the first stamp).  A frame of a device without an extractor uses the default one
 *   when no other device has one, and is ignored otherwise, as in the reference.
 * - lsa_slam_set_extractor_param = SetKeyPointsExtractor(extractor, deviceId) + the extractor's setter `name`
 *   ("NeighborWidth" ... "EdgeIntensityGapThreshold", "AzimuthalResolution"); device 0 always has an extractor.
 * - lsa_slam_set_base_to_lidar_offset / get = SetBaseToLidarOffset / GetBaseToLidarOffset(deviceId): rigid transform
 *   from the sensor to BASE (identity for a device nobody configured), device_id in [0, 255]. */
int lsa_slam_add_frames(lsa_slam* s, const lsa_point_t* const* pts, const int* n, const uint64_t* stamp_us, const uint32_t* seq, int nframes);
int lsa_slam_set_extractor_param(lsa_slam* s, int device_id, const char* name, double value);
int lsa_slam_get_extractor_param(const lsa_slam* s, int device_id, const char* name, double* value);
int lsa_slam_set_base_to_lidar_offset(lsa_slam* s, const double T[16], int device_id);
int lsa_slam_get_base_to_lidar_offset(const lsa_slam* s, double T[16], int device_id);
int lsa_slam_set_world_transform_from_guess(lsa_slam* s, const double T[16]);
int lsa_slam_get_trajectory(const lsa_slam* s, double* poses, double* covariances, int capacity);
int lsa_slam_get_debug_information(lsa_slam* s, double out[10]);
int lsa_slam_get_map(lsa_slam* s, int type, int clean, lsa_point_t* out, int capacity);
int lsa_slam_get_target_submap(lsa_slam* s, int type, lsa_point_t* out, int capacity);
lsa_ctx* lsa_slam_context(lsa_slam* s);
/* Slam::AddWheelOdomMeasurement / AddGravityMeasurement / ClearSensorMeasurements (Slam.cxx:1582-1598).  Weights and the
 * time offset are the parameters "WheelOdomWeight", "GravityWeight" and "SensorTimeOffset" of lsa_slam_set_param. */
int lsa_slam_add_wheel_odom_measurement(lsa_slam* s, double time, double distance);
int lsa_slam_add_gravity_measurement(lsa_slam* s, double time, const double acc[3]);
int lsa_slam_clear_sensor_measurements(lsa_slam* s);
/* the sensor terms the last frame's localization solved with (both flags 0: none) */
int lsa_slam_sensor_terms(const lsa_slam* s, lsa_sensor_terms_t* out);
/* The keypoint maps as PCD files (Slam::SaveMapsToPCD / LoadMapsFromPCD, Slam.cxx:504-543; formats: PCDFormat,
 * PointCloudStorage.h:60-65), one file per keypoint type: <prefix>edges.pcd, <prefix>planes.pcd, <prefix>blobs.pcd.
 * - lsa_slam_save_maps_pcd writes GetMap(k, filtered) of every keypoint type in use; an empty map writes no file.
 * - lsa_slam_load_maps_pcd: ClearMaps first when reset_maps != 0; then every file that exists goes into its map as ONE
 *   RollingGrid::Add(cloud, fixed, time) -- fixed when "MapUpdate" is NONE or ADD_KPTS_TO_FIXED_MAP, time < 0 = the wall
 *   clock in whole seconds (std::time(nullptr)); a file that does not exist leaves its map alone, a malformed one is an error.
 * - lsa_slam_add_map_points: that Add for points of the caller's (what the loader sits on).
 * All wait for the map workers, as the map getters do; the two that change a map drop what the look-ahead had prepared from
 * the maps as they were.  With the maps on the device (the default) a file is converted on the device
 * (lsa_device_grid_add_pcd / _save_pcd); with "MapsOnDevice" = 0 on the host.
 * - lsa_slam_map_io_counts: points per type of the last save / load, -1 where no file was written / found. */
int lsa_slam_add_map_points(lsa_slam* s, int type, const lsa_point_t* pts, int n, int fixed, double time);
int lsa_slam_save_maps_pcd(lsa_slam* s, const char* prefix, int format, int filtered);
int lsa_slam_load_maps_pcd(lsa_slam* s, const char* prefix, int reset_maps, double time);
int lsa_slam_map_io_counts(const lsa_slam* s, int counts[3]);
/* A trajectory corrected after the fact -- by GPS, a loop closure, g2o, GTSAM, Ceres, control points: any optimizer of the
 * caller's, or lsa_slam_optimize_logged_trajectory below for loop-closure edges -- brought back into the library: everything Slam::RunPoseGraphOptimization does AFTER its optimizer
 * (Slam.cxx:404-477).  Needs the keypoint log, i.e. "LoggingTimeout" != 0 while the frames were added (lsa_kplog_* above).
 * - lsa_slam_set_trajectory_and_rebuild_maps(poses17, n): rows as lsa_slam_get_trajectory gives them (row-major 4x4 + time).
 *   Waits for the map workers and the look-ahead; Reset(false); replaces the logged poses; re-projects every logged frame's
 *   raw keypoints under them (lsa_kplog_replay: per-point interpolation between consecutive poses unless "Undistortion" is
 *   NONE); per keypoint type in use ONE RollingGrid::Add(aggregate, fixed = false, time = -1, roll = false) and a Roll onto
 *   the last frame's box, on the device maps or ("MapsOnDevice" = 0) the host maps; Tworld = pose[n-1], PreviousTworld =
 *   pose[n-2].  The covariance log is kept.  The next lsa_slam_add_frame goes on as after lsa_slam_reset(s, 0).
 *   LSA_E_STATE when "LoggingTimeout" is 0, when keypoint logging stopped (a chunk could not be allocated; until
 *   lsa_slam_reset(s, 1)) or when the keypoint log does not cover the logged poses (logging was switched on in between);
 *   LSA_E_ARG when n is not the number of logged poses, n < 2, or a row's time is not the logged pose's.  On any of these
 *   nothing was changed.  A log of any length is taken, on the device maps as on the host maps: what remains is what one
 *   replay and one insertion address, 2^31 - 1 logged keypoints of one type (lsa_kplog_replay_to_grids, LSA_E_CAPACITY).
 * - lsa_slam_logged_frames: frames in the keypoint log; lsa_slam_get_logged_keypoints: one frame's raw keypoints of one
 *   type (returns their number, writes at most capacity).  Read-only parameter "LoggedKeypointsBytes": device memory held. */
int lsa_slam_set_trajectory_and_rebuild_maps(lsa_slam* s, const double* poses17, int n);
int lsa_slam_logged_frames(const lsa_slam* s);
int lsa_slam_get_logged_keypoints(lsa_slam* s, int frame, int type, lsa_point_t* out, int capacity);
/* Loop closure: the registration of a logged frame against the part of the log recorded when the place was first seen -- the
 * constraint a pose-graph optimizer (the caller's, or lsa_slam_optimize_logged_trajectory) takes; the corrected trajectory
 * comes back through lsa_slam_set_trajectory_and_rebuild_maps.  Nothing but the result leaves the device.
 * - lsa_slam_register_logged_frames(query q, revisited r, params, guess, out), indices into the logged trajectory:
 *   1. windows R = [r - revisited_half_window, r + ...] and Q = [q - query_half_window, q + ...], clipped to the log;
 *   2. target: per keypoint type in use the points of R under the logged poses (lsa_kplog_replay_range, rule 2 -- rule 0 when
 *      "Undistortion" is NONE) as ONE RollingGrid::Add(fixed = false, time = -1, roll = true) into a fresh device grid with
 *      that type's map parameters; the whole grid, unfiltered, is the kNN target;
 *   3. query: the points of Q under inv(P[q]) * P[i], same rule -- q's BASE frame;
 *   4. the ICP loop of Slam::Localization (match parameters, saturation distance interpolated over the iterations, types in
 *      the order EDGE, PLANE, BLOB, early end when a solve makes no step, skipped below "MinNbMatchedKeypoints", "TwoDMode"
 *      honoured) without sensor terms and without undistortion between the iterations, then the registration error.
 *   guess: row-major 4x4 world pose of q's BASE the loop starts from; NULL = the logged pose of q.  params NULL = defaults.
 *   All of it runs on a scratch context of the handle (made by the first call): the working keypoints, the map targets, the
 *   sub-maps' validity, the maps and the look-ahead of the frame path are not touched; the call waits for the map workers
 *   and for the device (it is an offline call).
 *   LSA_E_STATE when "LoggingTimeout" is 0, keypoint logging stopped, or the keypoint log does not cover the logged poses;
 *   LSA_E_ARG for an index outside the log, a negative window, or windows that overlap.  A refusal changes nothing.
 *   Read-only parameters of lsa_slam_get_param, a measurement hook: "LoopClosureReplaySeconds", "LoopClosureMapsSeconds",
 *   "LoopClosureIcpSeconds", "LoopClosureSeconds" -- the last call's two replays, scratch maps, ICP loop and the whole of it by the
 *   HOST's clock.  A stage counts what the host waited for in it: the replays are waited for, the insertions behind the first
 *   are only enqueued there and are waited for through the sub-maps' sizes, so their time is in the "maps" share.
 * - lsa_loop_closure_params_init: revisited_half_window 5, query_half_window 0, everything else 0.
 * - lsa_loop_closure_candidate(poses17, n, query, min_travelled, max_distance): host only, no device.  Rows as
 *   lsa_slam_get_trajectory gives them.  Among the frames i < query at least min_travelled metres back along the trajectory
 *   (sum of the step lengths between i and query) and at most max_distance metres from query's position, the nearest one,
 *   the lower index on a tie; -1 when there is none, LSA_E_ARG for a bad argument.  It decides by position alone; by
 *   appearance, drift or no drift, and with a yaw to start the registration from: lsa_slam_recognize_place below. */
typedef struct lsa_loop_closure_params_t
{
  int32_t revisited_half_window; /* frames on either side of `revisited` that make the target (default 5) */
  int32_t query_half_window;     /* frames on either side of `query` that are registered together (default 0) */
  int32_t icp_max_iter;          /* <= 0: "LocalizationICPMaxIter" */
  int32_t lm_max_iter;           /* <= 0: "LocalizationLMMaxIter" */
  double init_saturation;        /* <= 0: "LocalizationInitSaturationDistance" */
  double final_saturation;       /* <= 0: "LocalizationFinalSaturationDistance" */
} lsa_loop_closure_params_t;
typedef struct lsa_loop_closure_result_t
{
  double world[16];        /* the registered world pose of query's BASE, row-major */
  double relative[16];     /* inv(P[revisited]) * world: the edge revisited -> query */
  double covariance[36];   /* LocalOptimizer::EstimateRegistrationError at `world` (DoF order X, Y, Z, rX, rY, rZ) */
  double position_error;   /* [m] */
  double orientation_error;/* [deg] */
  int32_t status;          /* 0 registered; 1 skipped (fewer matches than "MinNbMatchedKeypoints"): world = the guess */
  int32_t iterations;      /* ICP iterations run */
  int32_t first_histogram[3][LSA_MATCH_NSTATUS]; /* match rejection histograms of the first ... */
  int32_t last_histogram[3][LSA_MATCH_NSTATUS];  /* ... and of the last iteration, per keypoint type */
  int64_t target_points[3];/* size of the target sub-map per keypoint type */
  int64_t query_points[3]; /* keypoints registered per type */
} lsa_loop_closure_result_t;
void lsa_loop_closure_params_init(lsa_loop_closure_params_t* params);
int lsa_slam_register_logged_frames(lsa_slam* s, int query, int revisited, const lsa_loop_closure_params_t* params, const double guess[16],
                                    lsa_loop_closure_result_t* out);
int lsa_loop_closure_candidate(const double* poses17, int n, int query, double min_travelled, double max_distance);

/* Place recognition on the keypoint log: which logged frame looks like this one, wherever the drifted trajectory puts it.
 * Every logged frame gets a descriptor made of its raw keypoints in its own coordinates (Scan Context, Kim & Kim, IROS
 * 2018): `rings` x `sectors` polar cells around the sensor, each the largest z + height_offset of the keypoints in it
 * (0 when empty or not positive), followed by the `sectors` column norms.  Two descriptors are compared column by column
 * under every column shift; the best shift is the yaw between the frames.  The definition, to the order of every float
 * operation, is lidarslam_amd/csrc/lsa_scan_descriptor.h, compiled for the host and the device alike.
 * - lsa_place_params_t: rings 1..32 (default 20), sectors 1..120 (60), type_mask a non-empty subset of the three types (EDGE
 *   and PLANE), min_range (0) < max_range (80), height_offset finite (2.0), min_common_sectors (15; <= 0: max(1, sectors / 4)):
 *   under a shift with fewer columns occupied in both descriptors the distance is 1.  Anything else: LSA_E_ARG.
 * - host statement, no device: lsa_scan_descriptor_host (n points already filtered by type -> rings * sectors + sectors
 *   floats), lsa_place_distance_host (query a, candidate b -> distance in [0, 2] and shift in [0, sectors)),
 *   lsa_place_select_host: from a table of (distance, shift) for the frames 0..query-1 and the trajectory (rows of 17 doubles)
 *   the admissible frames -- at least min_travelled back along the trajectory (lsa_loop_closure_candidate's rule), within
 *   max_distance of query's position if max_distance > 0, distance <= max_descriptor_distance if that is > 0 -- ranked by
 *   (distance, index); a frame within exclusion_half_window of one already picked is passed over.  Returns how many of at
 *   most `capacity` were written.  yaw = shift * 2 pi / sectors in (-pi, pi]: a start guess for
 *   lsa_slam_register_logged_frames is P[frame] * Rz(yaw).
 * - lsa_slam_recognize_place(query, search, out, capacity): describes the logged frames that have no descriptor yet
 *   (k_log_describe, a workgroup per frame), compares frame `query` with every frame before it (k_place_search, a workgroup per
 *   candidate, exhaustive and exact), copies the table out and selects on the host.  Returns the number of candidates.
 *   Runs on the log's context; waits for the map workers and the device (an offline call); changes nothing the frame path
 *   reads.  search NULL = defaults.  LSA_E_STATE when "LoggingTimeout" is 0, keypoint logging stopped, or the keypoint
 *   log does not cover the logged poses; LSA_E_ARG for a query outside the log or bad parameters. */
typedef struct lsa_place_params_t
{
  int32_t rings;
  int32_t sectors;
  uint32_t type_mask;          /* bit k: keypoints of type k take part */
  int32_t min_common_sectors;
  double min_range;            /* [m] horizontal range r with min_range <= r < max_range */
  double max_range;
  double height_offset;        /* [m] added to z: the sensor's height above the lowest thing worth describing */
} lsa_place_params_t;
typedef struct lsa_place_search_t
{
  lsa_place_params_t descriptor;
  double min_travelled;           /* [m] (default 20) */
  double max_distance;            /* [m] <= 0: no position gate (default 0) */
  double max_descriptor_distance; /* <= 0: no descriptor gate (default 0) */
  int32_t exclusion_half_window;  /* frames (default 5) */
  int32_t reserved;
} lsa_place_search_t;
typedef struct lsa_place_candidate_t
{
  int32_t frame;
  int32_t shift;
  float distance;
  float reserved;
  double yaw;                     /* [rad] */
} lsa_place_candidate_t;
void lsa_place_params_init(lsa_place_params_t* params);
void lsa_place_search_init(lsa_place_search_t* search);
int lsa_scan_descriptor_host(const lsa_place_params_t* params, const lsa_point_t* pts, int n, float* out);
int lsa_place_distance_host(const lsa_place_params_t* params, const float* a, const float* b, float* distance, int* shift);
int lsa_place_select_host(const float* distance, const int32_t* shift, const double* poses17, int n, int query, int sectors, double min_travelled,
                          double max_distance, double max_descriptor_distance, int exclusion_half_window, lsa_place_candidate_t* out, int capacity);
int lsa_slam_recognize_place(lsa_slam* s, int query, const lsa_place_search_t* search, lsa_place_candidate_t* out, int capacity);

/* Loop detection over the whole log: every place this drive revisited, in one call.
 * - A query set is first_query, first_query + query_stride, ... <= last_query (last_query < 0: the last logged frame;
 *   query_stride >= 1).  The result for query q is BY DEFINITION what lsa_place_select_host returns for q, with capacity
 *   per_query (1..16), from the table lsa_place_distance_host(D[q], D[i]), i = 0..q-1, under the same lsa_place_search_t.  The
 *   result of the call is the concatenation over the queries, ascending: records {query, frame, shift, distance, yaw}.  A
 *   query without an admissible frame contributes nothing; no candidate at all is an answer (0), not an error.
 * - lsa_loop_detect_init: lsa_place_search_init, first_query 0, last_query -1, query_stride 1, per_query 1.
 * - lsa_place_detect_host(detect, descriptors, poses17, n, out, capacity): the host statement, no device -- n descriptors of
 *   rings * sectors + sectors floats and n rows of 17 doubles; literally the loop over lsa_place_distance_host and
 *   lsa_place_select_host.  The gates and the ranking are lidarslam_amd/csrc/lsa_place_select.h, compiled for the device too.
 * - lsa_slam_detect_loop_closures(detect, out, capacity): the same for the keypoint log, on the device: the frames without a
 *   descriptor are described, many queries are compared in one pass over the descriptor store (k_place_search_rows), the
 *   selection runs on the device too (k_place_select_rows), and only the candidates come back -- one copy, one wait.  Equal
 *   to lsa_slam_recognize_place called for every query of the set, byte for byte.  Runs on the log's context after the map
 *   workers; changes nothing the frame path reads.  detect NULL = defaults.
 * All three return the number of candidates written.  LSA_E_ARG, with nothing written: a query set that is not one of this
 * log, per_query outside 1..16, capacity below queries * per_query, parameters out of limits.  LSA_E_STATE as
 * lsa_slam_recognize_place. */
typedef struct lsa_loop_detect_t
{
  lsa_place_search_t search;
  int32_t first_query;            /* (default 0) */
  int32_t last_query;             /* < 0: the last logged frame (default -1) */
  int32_t query_stride;           /* >= 1 (default 1) */
  int32_t per_query;              /* candidates a query, 1..16 (default 1) */
} lsa_loop_detect_t;
typedef struct lsa_loop_candidate_t
{
  int32_t query;
  int32_t frame;
  int32_t shift;
  float distance;
  double yaw;                     /* [rad] */
} lsa_loop_candidate_t;
void lsa_loop_detect_init(lsa_loop_detect_t* detect);
int lsa_place_detect_host(const lsa_loop_detect_t* detect, const float* descriptors, const double* poses17, int n, lsa_loop_candidate_t* out, int capacity);
int lsa_slam_detect_loop_closures(lsa_slam* s, const lsa_loop_detect_t* detect, lsa_loop_candidate_t* out, int capacity);

/* Place recognition against the MAPS: where in a loaded map is the vehicle, when nobody can say.  A saved
 * map has no logged frames to compare with, only points; what is compared with the last frame's descriptor is the descriptor
 * of the map AS SEEN FROM A VIEWPOINT, made for many viewpoints at once.
 * - A viewpoint is a position v (three doubles) in the maps' frame; its axes are the maps' axes.  LIMIT: the BASE is assumed
 *   level there -- roll and pitch are ignored.  A map point p takes part as the frame point x = (float)((double)p.x - v.x),
 *   likewise y and z (lsa_scan_descriptor.h: map_coord); from there on the descriptor is the frame descriptor's, verbatim:
 *   the descriptor of the map at v is lsa_scan_descriptor_host of the translated points of every map in type_mask --
 *   unfiltered Get content, any order (a cell holds a maximum), a NaN takes no part.
 * - The query is the last frame's raw keypoints in BASE (LSA_SET_RAW_CURRENT), the types of type_mask, described as a logged
 *   frame is; distance, shift and yaw are those of "Place recognition" above.  A candidate's start guess for the localization
 *   is Translation(v) * Rz(yaw): lsa_slam_set_world_transform_from_guess(candidate.guess).
 * - host statement, no device: lsa_map_descriptor_host, and lsa_map_place_select_host: from a table of (distance, shift) for
 *   V viewpoints (rows of three doubles) the admissible ones -- distance <= max_descriptor_distance if that is > 0, within
 *   max_distance of near_xyz (a GPS fix, the last good pose) if max_distance > 0, a NaN distance never -- ranked by
 *   (distance, index); a viewpoint within exclusion_radius metres (<=; only if exclusion_radius > 0) of one already picked is
 *   passed over.  Returns how many of at most `capacity` were written.  search NULL = defaults.  LSA_E_ARG: V < 1, a
 *   viewpoint or a search field that is not finite, sectors outside 1..120, no room.
 * - lsa_slam_recognize_place_in_maps(viewpoints, V, search, out, capacity, summary): waits for the map workers, describes
 *   the maps at the viewpoints on the device (k_map_describe; only when the descriptor's parameters, the viewpoints -- compared
 *   by content -- or a used map changed since the last call: summary->described says how many viewpoints this call
 *   described), describes the query, searches (k_place_search, exhaustive and exact) and selects on the host.  Returns the
 *   number of candidates.  Changes nothing the next frame relies on, and does not move the pose.  LSA_E_STATE, with the
 *   reason in lsa_slam_last_error, when no frame has been added since construction, Reset or SetWorldTransformFromGuess (the
 *   raw keypoints are empty), or when every map in the mask is empty; LSA_E_ARG as the host statement. */
typedef struct lsa_map_place_search_t
{
  lsa_place_params_t descriptor;
  double max_descriptor_distance; /* <= 0: no descriptor gate (default 0) */
  double exclusion_radius;        /* [m] <= 0: none (default 5) */
  double near_xyz[3];             /* [m] in the maps' frame; read only when max_distance > 0 */
  double max_distance;            /* [m] <= 0: no position gate (default 0) */
} lsa_map_place_search_t;
typedef struct lsa_map_place_candidate_t
{
  int32_t viewpoint;
  int32_t shift;
  float distance;
  float reserved;
  double yaw;                     /* [rad] */
  double guess[16];               /* row-major Translation(viewpoint) * Rz(yaw) */
} lsa_map_place_candidate_t;
typedef struct lsa_map_place_summary_t
{
  int32_t viewpoints;
  int32_t described;              /* viewpoints this call described (0: the table was kept) */
  int64_t map_points[3];          /* points of each map that were described (0 for a type outside the mask) */
  int64_t query_points[3];        /* keypoints of the query per type (0 for a type outside the mask) */
} lsa_map_place_summary_t;
void lsa_map_place_search_init(lsa_map_place_search_t* search);
int lsa_map_descriptor_host(const lsa_place_params_t* params, const lsa_point_t* pts, int n, const double viewpoint[3], float* out);
int lsa_map_place_select_host(const float* distance, const int32_t* shift, const double* viewpoints, int V, int sectors, const lsa_map_place_search_t* search,
                              lsa_map_place_candidate_t* out, int capacity);
int lsa_slam_recognize_place_in_maps(lsa_slam* s, const double* viewpoints, int V, const lsa_map_place_search_t* search, lsa_map_place_candidate_t* out, int capacity,
                                     lsa_map_place_summary_t* summary);


/* ------------------------------------------------------------------------- */
/* LidarSlam::RollingGrid ON THE DEVICE (slam_lib/include/LidarSlam/RollingGrid.h:63-212, slam_lib/src/RollingGrid.cxx): the
 * rolling voxel map of one keypoint type as ONE array of voxels sorted by (outer voxel index, leaf voxel index), living
 * in the memory of the context it was created on.  Add / Roll / ClearOldPoints / BuildSubMapKdTree are sequences of
 * kernels on the context's look-ahead stream (runs of the batch sorted in LDS and merged by rank, one thread per voxel
 * folding the batch's points for it in arrival order through the reference's per-point rule, old and new voxels merged
 * by rank, stable compactions), ordered by events against the context's stream wherever the two share data; the sub-map is written straight into a kNN target of the context.
 * One grid is driven by one host thread at a time (not necessarily the context's).  The order in which Get and the
 * sub-maps hand the points out is "Ordered" (the host grid's SetOrdered, lsa_slam's "OrderedMaps"):
 *   1 (default) KEY ORDER (outer index, then leaf index) -- a defined order in place of the reference's accidental one,
 *               adopted by the oracle and the host grid as well;
 *   0           the reference's own: the iteration order of its unordered_map<int, unordered_map<int, Voxel>>.  Every
 *               modification's effect on the key set goes to the host behind it (a few thousand keys per keyframe, an
 *               async copy and an event); the host replays it on a keys-only copy of those containers and uploads the
 *               keys in their iteration order before the next extraction.  The points never leave the device.
 *   Set on an empty grid, the order is exact from the first insertion on (from containers never used: set it before
 *   the first insertion).  Set while the grid holds points, the grid puts its points back in, in the order it hands
 *   them out now, the way the geometry setters do (Get, Clear, Add: counts start again, the points come back with
 *   time -1 and not fixed, so a map with a "DecayingThreshold" drops them at its next ClearOldPoints -- the host grid,
 *   whose SetOrdered only changes the order, keeps them).
 * Sampling modes FIRST, LAST, MAX_INTENSITY, CENTER_POINT, CENTROID.  Parameters by the reference's setter names:
 * "GridSize", "VoxelResolution", "LeafSize", "MinFramesPerVoxel", "Sampling", "DecayingThreshold", and "Ordered".
 * lsa_device_grid_set also takes "GlobalScans", a TEST KNOB that changes no result: which of its two forms an insertion
 * takes is a matter of its size (the chunk tables of the merge in LDS while they fit -- points / 256 + voxels / 1024 + 2 <=
 * 12 288, every keyframe's insertion --, scanned into global memory by launches of their own otherwise); 1 takes the second
 * form at any size, 2 takes it with scan blocks of 64 entries instead of 256, so that a further level of the scan is
 * reached with a million points; 0 (default) goes by size.  lsa_device_grid_get_param also answers "Voxels": the voxels the
 * map holds (the size of Get(false)) as of the last modification, which it waits for. */
typedef struct lsa_device_grid lsa_device_grid;
int lsa_device_grid_create(lsa_ctx* ctx, lsa_device_grid** out);
void lsa_device_grid_destroy(lsa_device_grid* g); /* before lsa_ctx_destroy of its context */
int lsa_device_grid_set(lsa_device_grid* g, const char* name, double value);
double lsa_device_grid_get_param(const lsa_device_grid* g, const char* name);
/* RollingGrid::Reset(position) / Clear(). */
int lsa_device_grid_reset(lsa_device_grid* g, const float position[3]);
int lsa_device_grid_clear(lsa_device_grid* g);
/* RollingGrid::Size() (waits for the modifications enqueued so far). */
int lsa_device_grid_size(lsa_device_grid* g);
/* RollingGrid::Add(pointcloud, fixed, currentTime, roll) from host points ...  One call is one Add whatever its size (a
 * voxel's frame count rises once, the sampling modes see the whole cloud in arrival order).  LSA_E_CAPACITY when the voxels
 * of the map and the points of the insertion together are more than 2^31 - 8193, what the kernels address. */
int lsa_device_grid_add(lsa_device_grid* g, const lsa_point_t* pts, int n, int fixed, double time, int roll);
/* ... and from a keypoint set of the context moved by `pose` (Slam::UpdateMapsUsingTworld, Slam.cxx:1178-1222): nothing
 * leaves the device and nothing is waited for. */
int lsa_device_grid_add_keypoints(lsa_device_grid* g, int set, int type, const double pose[16], double time);
/* The same in two steps, for a caller that hands the insertion proper to another host thread: _stage_keypoints (on the
 * context's thread) reads the keypoints -- the set may be rewritten right after --, _add_staged inserts them. */
int lsa_device_grid_stage_keypoints(lsa_device_grid* g, int set, int type, const double pose[16]);
int lsa_device_grid_add_staged(lsa_device_grid* g, double time);
/* _stage_keypoints for the keypoint types of a keyframe together (grids[i] takes type types[i] of the set): one launch */
int lsa_device_grid_stage_keypoints_all(lsa_device_grid* const* grids, const int* types, int count, int set, const double pose[16]);
/* ... for up to three maps of one context at once: one launch of every step serves all of them (a block row per map). */
int lsa_device_grid_add_staged_all(lsa_device_grid* const* grids, int count, double time);
int lsa_device_grid_roll(lsa_device_grid* g, const float min_point[3], const float max_point[3]);
int lsa_device_grid_clear_old_points(lsa_device_grid* g, double current_time);
/* RollingGrid::Get(clean): points written. */
int lsa_device_grid_get(lsa_device_grid* g, int clean, lsa_point_t* out, int capacity);
/* RollingGrid::BuildSubMapKdTree(): the sub-map (the whole map when min_point == NULL) becomes the kNN target (slot,
 * type) of the context; returns its size.  lsa_device_grid_submap_valid: RollingGrid::IsSubMapKdTreeValid(). */
int lsa_device_grid_build_submap(lsa_device_grid* g, const float min_point[3], const float max_point[3], int min_nb_points, int slot, int type);
/* The same in two steps: _begin enqueues the extraction, _end waits for it and returns the size -- several grids build
 * side by side.  _begin_for_keypoints takes the box of keypoint type `box_type` as lsa_keypoint_bboxes_begin (which must
 * come right before, and needs no lsa_keypoint_bboxes_end then) left it on the device: nothing is read back. */
int lsa_device_grid_build_submap_begin(lsa_device_grid* g, const float min_point[3], const float max_point[3], int min_nb_points, int slot, int type);
int lsa_device_grid_build_submap_begin_for_keypoints(lsa_device_grid* g, int box_type, int min_nb_points, int slot, int type);
int lsa_device_grid_build_submap_end(lsa_device_grid* g);
int lsa_device_grid_submap_valid(lsa_device_grid* g);
/* Sub-maps AHEAD of time.  The sub-map only depends on the outer voxels the keypoints' box touches, and the predicted pose
 * gives that box to a voxel long before the localization asks: _ahead_begin (right after lsa_keypoint_bboxes_begin(_interp)
 * under the PREDICTED pose, no lsa_keypoint_bboxes_end) extracts the sub-map for the box of keypoint type `box_type` into
 * the context's spare map target, behind the grid's last insertion; _ahead_poll (non-blocking; returns 0 nothing, 1
 * extraction on its way, 2 search grid enqueued) is called now and then meanwhile (or _ahead_wait from a thread of its own); _ahead_take (right after
 * lsa_keypoint_bboxes_begin under the ACTUAL pose) compares the two voxel ranges on the device: when they are the same the
 * spare target becomes target (slot, type), *taken = 1 and the size is returned; otherwise *taken = 0 and the caller
 * extracts the sub-map as usual.  The same sub-map either way. */
int lsa_device_grid_submap_ahead_begin(lsa_device_grid* g, int box_type, int min_nb_points, int type);
int lsa_device_grid_submap_ahead_poll(lsa_device_grid* g);
/* ... of several maps of one context: when all their sizes have arrived, their search grids are built by one sequence of
 * launches (1 while a size is missing, 2 when done). */
int lsa_device_grid_submap_ahead_poll_all(lsa_device_grid* const* grids, int count);
int lsa_device_grid_submap_ahead_wait(lsa_device_grid* g); /* blocking form of _poll, for a thread with nothing else to do */
int lsa_device_grid_submap_ahead_take(lsa_device_grid* g, int box_type, int min_nb_points, int slot, int type, int* taken);
/* _take in two steps (several maps: every comparison is enqueued before any is waited for): _take_begin returns 1 when a
 * comparison is on its way, 0 when nothing fits; _take_end waits for it. */
int lsa_device_grid_submap_ahead_take_begin(lsa_device_grid* g, int box_type, int min_nb_points, int slot, int type);
int lsa_device_grid_submap_ahead_take_end(lsa_device_grid* g, int* taken);
/* A PCD file into the map and the map into a PCD file; the conversion between the file's records and LidarPoints runs on
 * the device (k_pcd_decode / k_pcd_encode), ascii text and the LZF stage on the host.
 * - lsa_device_grid_add_pcd = RollingGrid::Add(the file's cloud, fixed, time, roll_first), the whole file as ONE Add; the
 *   data section goes up in pieces through pinned staging on the context's copy stream, piece i is converted while piece
 *   i + 1 is uploaded.  A malformed file: LSA_E_ARG, lsa_last_error names the file and the line.  A file of any size the
 *   format counts (2^31 - 1 points) and lsa_device_grid_add addresses is taken.
 * - lsa_device_grid_save_pcd writes RollingGrid::Get(clean) in the order lsa_device_grid_get hands it out; returns the
 *   number of points written: 0, and no file, when there is none (an empty cloud is not saved, PointCloudStorage.h:91-92);
 *   every failure -- a path that cannot be written among them -- is negative and lsa_last_error names the file.
 * - lsa_pcd_io_times: seconds of the context's last load / save: [0] file, [1] LZF, [2] text, [3] pieces on their way
 *   (upload or download + conversion), [4] the grid's Add / Get, [5] bytes moved, [6] points; [3] and [4] wait for the
 *   device only while profiling is on (scopes "pcd_upload", "pcd_decode", "pcd_encode", "map_add"). */
int lsa_device_grid_add_pcd(lsa_device_grid* g, const char* path, int fixed, double time, int roll_first);
int lsa_device_grid_save_pcd(lsa_device_grid* g, const char* path, int format, int clean);
int lsa_pcd_io_times(const lsa_ctx* ctx, double out[8]);

/* ------------------------------------------------------------------------- */
/* The dense point-cloud map: registered frames voxel-hashed on the device (lsa_dense_*.hip).  The keypoint
 * maps above are the ICP's target; this is the point cloud of the place, one LidarPoint per voxel of `leaf` metres, built
 * from whole registered frames without any of them leaving the device.  The host statement it is held to byte for byte is
 * DenseMapHost (lidarslam_amd/_dense_map.py):
 * - a point takes no part, and is counted in `skipped`, when a coordinate is not finite or an index i_a = floor((double)p_a /
 *   (double)leaf) lies outside [-2^20, 2^20); key = ((iz + 2^20) << 42) | ((iy + 2^20) << 21) | (ix + 2^20), ascending key is
 *   z-major order; -0.0 falls into voxel 0, -0.125 into voxel -1;
 * - within one call a voxel's winner is its point of largest intensity (compared by lsa_wave.h's ordered code: a NaN loses to
 *   every number, -0.0 to +0.0), ties to the smallest index of the call; n_f = the call's points in the voxel;
 * - a new voxel: point = the winner's 32 bytes, count = n_f, frames = 1, first_frame = last_frame = frame; an existing one:
 *   count += n_f, frames += 1 unless last_frame == frame, last_frame = frame, and the point is replaced only when the winner's
 *   intensity is strictly greater (the earlier frame keeps ties).
 * `frame` is an ordinal that must not decrease from one call to the next (LSA_E_ARG).  Nothing depends on the order in which
 * the points of one call arrive.
 * - lsa_dense_map_set: "MaxBytes" (of the table; default 16 GiB, 0 = no limit), "InitialCapacity" (slots of the table the
 *   next insertion into a map without one makes; rounded up to a power of two), "ProbeStress" (a TEST KNOB: every key's home
 *   slot is 0; only on an empty map).  lsa_dense_map_get_param also answers "LeafSize", "Capacity", "Rehashes", "ExportSeconds".
 * - _insert_points: world points of the caller's (the table alone).  _insert_frame: the context's current frame moved as
 *   lsa_transform_frame_at moves it, fused with the insertion: equal, byte for byte, to _insert_points of that call's
 *   download; nothing is waited for, and the frame's device buffer is held by an event until the insertion has read it.
 * - Growth: before an insertion the table is made large enough for (upper bound of occupied slots) + n <= capacity / 2, by a
 *   rehash into a table of twice the size on the same stream; the old one is freed by lsa_collect_garbage.  When that table
 *   would exceed "MaxBytes" (or cannot be allocated) the WHOLE insertion is refused with LSA_E_CAPACITY, lsa_last_error says
 *   why and the map is untouched: never a partial frame, never a silently dropped point.
 * - _size (voxels), _skipped, _get and _save_pcd wait for the insertions in flight.  _get returns the number of voxels with
 *   frames >= min_frames and writes at most `capacity` of them in ascending key order (pts or voxels may be NULL); _save_pcd
 *   writes the same points, returns their number, 0 and no file for none.  LSA_E_STATE when a probe sequence ran through
 *   the whole table (it is bounded by the capacity; cannot happen at load <= 1/2).
 * - Source: beside its record a voxel keeps `source`, the ordinal of the call whose point it holds (set when the voxel is made
 *   or its point replaced).  _get_sources returns them aligned with _get(min_frames), same order, same return convention.
 * - _reproject moves what the map kept under a corrected trajectory -- one point per voxel, moved by the correction of the
 *   frame that measured it; not a rebuild from raw frames, which are not logged: two neighbouring surface voxels may merge
 *   and the voxel between them may stay empty until it is seen again.  corrections16: n row-major 4x4 rigid transforms,
 *   entry j for ordinal first_frame + j; a voxel takes entry c = clamp(source - first_frame, 0, n - 1).  Its point moves as
 *   lsa_device_math.h's rigid_apply moves it, in double, without contraction, narrowed to float: x' = (float)(((R0 x + R1 y)
 *   + R2 z) + t0) and likewise y', z' (a -0.0 comes out +0.0 under the identity); the other 20 bytes are kept.  The new key
 *   is the moved point's; a moved point that is not finite or outside the index range drops its voxel (counted in *dropped
 *   and in "Dropped", not in `skipped`).  Voxels that arrive at one key merge: count the sum modulo 2^32, first_frame the
 *   min, last_frame the max, frames = min(sum of frames, last_frame - first_frame + 1), point and source from the voxel of
 *   largest intensity code, ties to the smaller source, then to the smaller old key.  Nothing depends on the order in which
 *   the voxels are visited; the guard on non-decreasing ordinals is unchanged and insertion goes on afterwards.  The call
 *   waits for the insertions in flight, builds a second table of the same capacity (the voxel count cannot grow) with three
 *   launches over the old slots and retires the old one; its cost is the map's size, not the drive's.  LSA_E_ARG for n < 1
 *   or a NULL pointer, LSA_E_CAPACITY when the second table cannot be allocated: the map is untouched by either.
 *   lsa_dense_map_get_param answers "Reprojections", "Dropped" (voxels, since the last clear), "ReprojectSeconds" (the last).
 * - lsa_pose_corrections: out_i = new_i * inverse(old_i) for n poses (row-major 4x4, rigid inverse R^T, -R^T t, in double):
 *   the corrections the pipeline hands _reproject.
 * - Free space (DenseMapHost.carve is the statement, and exact).  Beside `source` a voxel keeps `misses` (u32) and the last
 *   ordinal that counted one.  _carve_points: every point with index % "CarveStride" == 0 casts a ray from its origin
 *   (origins_xyz: n_origins = 1 or n float triples, world positions of the sensor) to the point, in double, without
 *   contraction: d = p - o, len = sqrt((dx*dx + dy*dy) + dz*dz), t = min(len - "CarveMarginLeaves" * leaf, "CarveRange");
 *   no ray when a coordinate is not finite, t is not > 0 or a start or end index is outside [-2^20, 2^20); e = o + d * (t /
 *   len), i0 = floor(o / leaf), i1 = floor(e / leaf); per axis left = |i1 - i0|, step = sign(i1 - i0), tmax = ((i0 + (step >
 *   0)) * leaf - o) / (e - o), tdelta = leaf / |e - o|; the ray visits i0 and then, left_x + left_y + left_z times, steps
 *   along the axis of smallest tmax among those with steps left (ties x, y, z) and visits: a 6-connected path that ends in
 *   i1.  A visited voxel that exists and whose last_frame and last counted ordinal both differ from `frame` takes one miss:
 *   once an ordinal, whatever the rays and calls, none in an ordinal that hit it -- so insert every frame of an ordinal before
 *   carving any.  Nothing depends on the order of the rays.  A carve makes, moves and removes no voxel and touches no point
 *   or record.  `frame` must not be below the map's last ordinal, nor -2^31 (LSA_E_ARG), and becomes the last.  One launch,
 *   one thread a ray, behind the insertions on the same stream; nothing is waited for.  _carve_frame: the context's current
 *   frame, fused as _insert_frame: the point is lsa_transform_frame_at's, the origin what that call makes of the frame's own
 *   (0, 0, 0) at the point's time (lsa_transform_frame_origins_at hands those out, float xyz per frame point): under
 *   undistortion every ray starts where the sensor was when it fired.  The frame's buffer is held until the carve has read it.
 *   lsa_dense_map_set: "CarveMarginLeaves" (default 2), "CarveRange" (metres, default 30; LSA_E_ARG above 4096 leaves: the
 *   bound of a ray's walk), "CarveStride" (default 1).  get_param: those, "Rays" (cast since the last clear), "Pruned"
 *   (voxels, since the last clear), "Prunes", "CarveSeconds" (the host's, of the last call).  The misses live in an array of
 *   8 B a slot made by the first carve (counted by _bytes, not by "MaxBytes"): a map never carved pays nothing.
 * - _get_filtered, _get_sources_filtered, _get_misses, _save_pcd_filtered: as _get and its neighbours, of the voxels with
 *   frames >= min_frames and, for max_miss_ratio >= 0, (double)misses <= max_miss_ratio * (double)frames; the calls without
 *   a ratio are these with -1.  _prune removes the other voxels for good: a rehash of what passes into a zeroed table of the
 *   smallest power-of-two capacity >= 64 with capacity / 2 >= the kept (the old one is freed by lsa_collect_garbage);
 *   *removed and "Pruned" count them, `skipped` and "Dropped" do not.  LSA_E_CAPACITY, the map untouched, without memory for
 *   the second table.  _reproject carries the state: merged voxels take the sum of the misses modulo 2^32 and the later
 *   ordinal. */
typedef struct lsa_dense_voxel_t
{
  uint64_t key;
  uint32_t count;       /* points that fell into the voxel */
  uint32_t frames;      /* frame ordinals that touched it */
  int32_t first_frame;
  int32_t last_frame;
} lsa_dense_voxel_t;
typedef struct lsa_dense_map lsa_dense_map;
int lsa_dense_map_create(lsa_ctx* ctx, double leaf, lsa_dense_map** out);
void lsa_dense_map_destroy(lsa_dense_map* dm); /* before lsa_ctx_destroy of its context */
int lsa_dense_map_set(lsa_dense_map* dm, const char* name, double value);
double lsa_dense_map_get_param(lsa_dense_map* dm, const char* name);
int lsa_dense_map_insert_points(lsa_dense_map* dm, const lsa_point_t* pts, int n, int frame);
int lsa_dense_map_insert_frame(lsa_dense_map* dm, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset, int frame);
int lsa_dense_map_reserve(lsa_dense_map* dm, long long n); /* room for n more points now, as an insertion of n would make it: LSA_E_CAPACITY as there */
int lsa_dense_map_size(lsa_dense_map* dm);
long long lsa_dense_map_skipped(lsa_dense_map* dm);
long long lsa_dense_map_bytes(const lsa_dense_map* dm);
int lsa_dense_map_get(lsa_dense_map* dm, int min_frames, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity); /* every export: LSA_E_CAPACITY without device memory for its scratch (keys, sort, columns) */
int lsa_dense_map_get_sources(lsa_dense_map* dm, int min_frames, int32_t* out, int capacity);
int lsa_dense_map_reproject(lsa_dense_map* dm, const double* corrections16, int first_frame, int n, long long* dropped);
int lsa_pose_corrections(const double* old16, const double* new16, int n, double* out16);
int lsa_dense_map_clear(lsa_dense_map* dm);
int lsa_dense_map_save_pcd(lsa_dense_map* dm, const char* path, int format, int min_frames);
int lsa_dense_map_carve_points(lsa_dense_map* dm, const lsa_point_t* pts, int n, const float* origins_xyz, int n_origins, int frame);
int lsa_dense_map_carve_frame(lsa_dense_map* dm, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset, int frame);
int lsa_transform_frame_origins_at(lsa_ctx* ctx, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset, float* xyz, int capacity);
int lsa_dense_map_get_filtered(lsa_dense_map* dm, int min_frames, double max_miss_ratio, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity);
int lsa_dense_map_get_sources_filtered(lsa_dense_map* dm, int min_frames, double max_miss_ratio, int32_t* out, int capacity);
int lsa_dense_map_get_misses(lsa_dense_map* dm, int min_frames, double max_miss_ratio, uint32_t* out, int capacity);
int lsa_dense_map_prune(lsa_dense_map* dm, int min_frames, double max_miss_ratio, long long* removed);
int lsa_dense_map_save_pcd_filtered(lsa_dense_map* dm, const char* path, int format, int min_frames, double max_miss_ratio);
/* Normals (DenseMapHost.normals is the statement, held byte for byte): one record per voxel of _get_filtered(min_frames,
 * max_miss_ratio), in its order, computed from the table as it stands -- nothing is stored, no state changes.  For a voxel of
 * index (ix, iy, iz) and point p the cells (ix+dx, iy+dy, iz+dz), dz, dy, dx in -radius_leaves .. radius_leaves with dx fastest,
 * are visited (none with an index outside [-2^20, 2^20)); a cell is a neighbour when its voxel exists and passes the same
 * predicate, the voxel itself among them.  In double, from +0.0, without contraction, in that order: d = q - p, s += d, S_ab
 * += d_a * d_b, k = neighbors.  k < min_neighbors: the four floats are the quiet NaN 0x7fc00000 (PCL's "no normal").  Else
 * C_ab = S_ab / k - (s_a / k) * (s_b / k), pcl::eigen33 in double gives l0 <= l1 <= l2 and e0 (not finite: that NaN); with
 * n_viewpoints > 0 the voxel takes viewpoint clamp(source - first_frame, 0, n_viewpoints - 1) and e0 is negated when (e0 .
 * (viewpoint - p)) < 0; normal = (float)e0, curvature = (float)|l0 / (l0 + l1 + l2)| (0 when the sum is not positive).
 * LSA_E_ARG, the map untouched: radius_leaves not 1 or 2, min_neighbors < 3 or > (2 radius_leaves + 1)^3, min_frames < 1,
 * n_viewpoints < 0 or viewpoints missing.  Two launches behind the export's compaction and sort (k_dense_normals: a group of 32
 * lanes a voxel for the sums; k_dense_normal_records: one thread a voxel for the rest), one upload of the viewpoints; the call
 * waits and returns the count under _get_filtered's capacity rules.
 * get_param: "NormalsSeconds" (the last call).  _save_pcd_normals: the points of _save_pcd_filtered with the fields normal_x
 * normal_y normal_z curvature behind the LidarPoint's eight (44-byte records; "nan" in ascii); lsa_pcd_read gives the points of
 * such a file as of any other, lsa_pcd_read_normals the four floats per point (LSA_E_ARG, the reason in lsa_pcd_last_error,
 * when one of the four fields is missing or is not a 4-byte F). */
typedef struct lsa_dense_normal_t
{
  float nx, ny, nz, curvature;
  uint32_t neighbors;
} lsa_dense_normal_t;
int lsa_dense_map_get_normals(lsa_dense_map* dm, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors, const float* viewpoints_xyz,
                              int n_viewpoints, int first_frame, lsa_dense_normal_t* out, int capacity);
int lsa_dense_map_save_pcd_normals(lsa_dense_map* dm, const char* path, int format, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors,
                                   const float* viewpoints_xyz, int n_viewpoints, int first_frame);
int lsa_pcd_read_normals(const char* path, float* out4, int capacity);
/* The floor plan (DenseMapHost.grid is the statement, held byte for byte): elevation, ground and a 2-D occupancy grid in the
 * convention of nav_msgs/OccupancyGrid, rasterised on the device from the table as it stands -- nothing is stored, no state
 * changes, nothing is launched on the frame path.  Only the voxels of _get_filtered(min_frames, max_miss_ratio) take part.  A
 * voxel of index (ix, iy, iz) belongs to cell (ix // cell_leaves, iy // cell_leaves), floor division.  Floats are compared by
 * their ordered codes (-0.0 below +0.0).  elevation: the kept point z of smallest code among the cell's voxels.  ground: the
 * smallest-code elevation over the (2 ground_radius + 1)^2 cells around that have a voxel, the cell among them, inside the
 * extent or not.  Per voxel h = (double)z - (double)ground(cell): h <= min_height counts in floor_voxels, min_height < h <=
 * max_height in obstacle_voxels (top: the obstacle z of largest code), anything higher is ignored.  state: 100 when
 * obstacle_voxels >= min_obstacle_voxels, else 0 when floor_voxels >= 1, else -1: free means the floor was seen.  A float that
 * is not there is the quiet NaN 0x7fc00000.
 * Extent: without a window the bounding box of the kept voxels' cells (none: width = height = 0, no error).  With use_window
 * the cells cx0 = floor(x_min / leaf) // cell_leaves .. floor(x_max / leaf) // cell_leaves, likewise in y, whatever the map
 * holds (a window wholly outside the index range [-2^20, 2^20) has no cell, any other is clamped to it): a window's answer
 * is the crop of the whole grid's.  resolution = cell_leaves * leaf, origin_x = (double)(cx0 * cell_leaves) * leaf; cells are
 * row-major, row 0 is cy0, x fastest.
 * _get_grid fills *info, writes min(cells, capacity) records and states (either output may be null; with both null only the
 * extent is computed) and returns width * height.  LSA_E_ARG, the map untouched: cell_leaves outside 1..64, ground_radius
 * outside 0..16, not (0 <= min_height < max_height, both finite), min_obstacle_voxels < 1, a window that is not finite or has
 * min > max, capacity < 0.  LSA_E_CAPACITY, before anything is allocated: width * height, formed in 64 bits, above
 * "GridMaxCells" (lsa_dense_map_set, 1 .. 2^28, default 2^24); also when the rasters cannot be allocated.
 * get_param: "GridMaxCells", "GridSeconds" (the last call).  _save_grid writes the states as <prefix>.pgm and <prefix>.yaml
 * for map_server (lsa_occupancy_write) and returns the number of cells; 0 and no files for none.
 * lsa_occupancy_write (host only): binary P5 of maxval 255 -- occupied 0, free 254, anything else 205 --, image row 0 the
 * grid's last row; the yaml holds image (the file's name), resolution, origin: [origin_x, origin_y, 0], negate: 0,
 * occupied_thresh: 0.65, free_thresh: 0.196.  LSA_E_ARG with the reason in lsa_occupancy_last_error (of the calling thread) when a
 * file cannot be written; nothing is written for a grid without cells. */
typedef struct lsa_dense_grid_params_t
{
  double min_height, max_height; /* metres above the ground: 0.2, 2.0 */
  double max_miss_ratio;         /* the export's filter; below 0: none */
  double window[4];              /* x_min, y_min, x_max, y_max in metres; read under use_window */
  int32_t cell_leaves;           /* 1..64: 2 */
  int32_t ground_radius;         /* cells, 0..16: 2 */
  int32_t min_obstacle_voxels;   /* >= 1: 1 */
  int32_t min_frames;            /* the export's filter: 1 */
  int32_t use_window;
} lsa_dense_grid_params_t;
typedef struct lsa_dense_grid_info_t
{
  int32_t cx0, cy0, width, height;
  double resolution, origin_x, origin_y;
} lsa_dense_grid_info_t;
typedef struct lsa_dense_cell_t
{
  float elevation, ground, top;
  uint32_t floor_voxels, obstacle_voxels;
} lsa_dense_cell_t;
long long lsa_dense_map_get_grid(lsa_dense_map* dm, const lsa_dense_grid_params_t* params, lsa_dense_grid_info_t* info, lsa_dense_cell_t* cells, int8_t* state,
                                 long long capacity);
long long lsa_dense_map_save_grid(lsa_dense_map* dm, const lsa_dense_grid_params_t* params, const char* prefix);
int lsa_occupancy_write(const char* prefix, const lsa_dense_grid_info_t* info, const int8_t* state);
const char* lsa_occupancy_last_error(void);
/* The pipeline's dense map (lsa_slam_set_param "DenseMap": 0 off, the default, under which nothing whatever changes; 1 every
 * registered frame; 2 keyframes only; "DenseMapLeafSize", default 0.1; "DenseMapMaxBytes"; read-only "DenseMapVoxels",
 * "DenseMapBytes", "DenseMapSkipped", "DenseMapRefusedFrames", "DenseMapClears").  At the end of AddFrame(s) the frame or frames of the
 * call are inserted under the poses lsa_slam_get_registered_frame would use, every device frame of one call with the same
 * ordinal, the count of inserted calls; room for all the device frames of a call is made before the first goes in, so a call
 * is inserted whole or refused whole (LSA_E_CAPACITY): a refused one counts in "DenseMapRefusedFrames", leaves its reason in
 * lsa_slam_last_error and does not fail the frame.  Also read-only: "DenseMapCapacity" (slots), "DenseMapFrames", "DenseMapRehashes",
 * "DenseMapExportSeconds".  The map is cleared by Reset, ClearMaps and everything that applies a corrected
 * trajectory (lsa_slam_set_trajectory_and_rebuild_maps; the pose-graph calls and lsa_slam_close_loops with `apply`): its
 * points were placed under the old poses and raw frames are not logged, so a stale map must not pass for a corrected one
 * ("DenseMapClears" counts, the first one warns on stderr), also while "DenseMap" is 0 for the moment.  The calls below wait for the insertions in flight and refuse
 * with LSA_E_STATE while "DenseMap" is 0.
 * "DenseMapOnTrajectory" (default 0: an applied trajectory clears, as said; 1: it re-projects): with 1 and a map that is not
 * empty, lsa_slam_set_trajectory_and_rebuild_maps -- and so every call that applies through it -- takes D_i = new_i *
 * inverse(old_i) per logged pose (lsa_pose_corrections, against the poses it actually applies), gives every dense ordinal
 * the correction of the logged pose dated like its frame (8 B a frame are kept for that; ordinals that have left the log under
 * a positive LoggingTimeout take the oldest logged pose's), and calls lsa_dense_map_reproject; "DenseMapFrames" is not reset
 * and mapping goes on with the next ordinal.  If the second table cannot be allocated the trajectory is applied all the same
 * and the map is cleared as under 0 ("DenseMapClears", the reason in lsa_slam_last_error).  Reset, ClearMaps,
 * lsa_slam_clear_dense_map and a changed leaf size clear under either value.  Read-only: "DenseMapReprojections",
 * "DenseMapDropped", "DenseMapReprojectSeconds".  _get_dense_map_sources: lsa_dense_map_get_sources of the pipeline's map.
 * Free space: "DenseMapCarve" (default 0: nothing changes, not a launch; 1: on), "DenseMapCarveRange", "DenseMapCarveMarginLeaves",
 * "DenseMapCarveStride" (lsa_dense_map_set's, same defaults); read-only "DenseMapRays", "DenseMapPruned".  With 1, once ALL device
 * frames of the call are inserted, all of them are carved (lsa_dense_map_carve_frame) under the same poses and the same ordinal,
 * so that a voxel the second LiDAR hit is not seen through by the first; a refused insertion carves nothing.  _filtered,
 * _misses, _save_..._filtered and _prune_dense_map are the map's calls of those names; the state survives "DenseMapOnTrajectory"
 * 1 and goes with everything that clears the map.  _get_registered_frame_origins: float xyz per point of
 * lsa_slam_get_registered_frame, in its order: where the sensor stood when it measured the point -- the origins of the carve. */
int lsa_slam_dense_map_size(lsa_slam* s);
int lsa_slam_get_dense_map(lsa_slam* s, int min_frames, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity);
int lsa_slam_get_dense_map_sources(lsa_slam* s, int min_frames, int32_t* out, int capacity);
int lsa_slam_save_dense_map_pcd(lsa_slam* s, const char* path, int format, int min_frames);
int lsa_slam_clear_dense_map(lsa_slam* s);
int lsa_slam_get_dense_map_filtered(lsa_slam* s, int min_frames, double max_miss_ratio, lsa_point_t* pts, lsa_dense_voxel_t* voxels, int capacity);
int lsa_slam_get_dense_map_misses(lsa_slam* s, int min_frames, double max_miss_ratio, uint32_t* out, int capacity);
int lsa_slam_save_dense_map_pcd_filtered(lsa_slam* s, const char* path, int format, int min_frames, double max_miss_ratio);
int lsa_slam_prune_dense_map(lsa_slam* s, int min_frames, double max_miss_ratio, long long* removed);
int lsa_slam_get_registered_frame_origins(lsa_slam* s, float* xyz, int capacity);
/* Normals of the pipeline's map: with "DenseMap" on, every inserted ordinal keeps its viewpoint (12 B a frame on the host): the
 * translation of Tworld * BaseToLidarOffset(device of the call's first frame), narrowed to float; what clears the map clears
 * the list, and under "DenseMapOnTrajectory" 1 an applied trajectory moves each viewpoint by the correction its ordinal's
 * voxels take, in the arithmetic of the re-projection.  _get_dense_map_viewpoints hands the list out (the count; *first_frame:
 * the ordinal of entry 0).  _get_dense_map_normals / _save_dense_map_pcd_normals: the map's calls, with these viewpoints
 * when `orient` is not 0 and none otherwise. */
int lsa_slam_get_dense_map_normals(lsa_slam* s, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors, int orient, lsa_dense_normal_t* out, int capacity);
int lsa_slam_save_dense_map_pcd_normals(lsa_slam* s, const char* path, int format, int min_frames, double max_miss_ratio, int radius_leaves, int min_neighbors, int orient);
int lsa_slam_get_dense_map_viewpoints(lsa_slam* s, float* xyz, int capacity, int* first_frame);
/* The floor plan of the pipeline's map: lsa_dense_map_get_grid / _save_grid behind the insertions in flight; "DenseMapGridMaxCells"
 * (lsa_slam_set_param) is the map's "GridMaxCells".  LSA_E_STATE while "DenseMap" is 0.  A map that no frame has reached yet
 * is an empty one. */
long long lsa_slam_get_dense_map_grid(lsa_slam* s, const lsa_dense_grid_params_t* params, lsa_dense_grid_info_t* info, lsa_dense_cell_t* cells, int8_t* state,
                                      long long capacity);
long long lsa_slam_save_dense_map_grid(lsa_slam* s, const lsa_dense_grid_params_t* params, const char* prefix);

/* Rays through the dense map (lsa_dense_cast.hip, DESIGN.md 3.14 "Rays"; the statement is DenseMapHost.cast / .compare, and the
 * device is held to its bytes).  A ray runs from an origin o towards a target t, both float widened to double, with the
 * geometry of the carve and len + extend in place of len - margin: tt = min(len + extend, max_range), e = o + (t - o) * (tt /
 * len); no ray when a coordinate is not finite, tt is not > 0, len is 0 or an end index lies outside [-2^20, 2^20).  The walk
 * is the carve's (one device function, dense_ray_begin / dense_ray_step).  A visited voxel counts when it exists, frames >=
 * min_frames, for max_miss_ratio >= 0 misses <= max_miss_ratio * frames (the export's predicate) and, under use_before,
 * first_frame < before.  The first that counts is the hit and ends the walk.  lsa_dense_hit_t: key (as lsa_dense_voxel_t's; 0
 * unless status 1), entry / exit = (float)(t_in * tt) / (float)(t_out * tt) -- metres along the ray at which it enters and
 * leaves the voxel --, depth = the kept point projected on the ray, steps = voxels visited (up to the hit; all for a miss; 0
 * for no ray), source = the hit voxel's source ordinal, status -1 no ray, 0 miss, 1 hit.  points (may be NULL): the hit
 * voxel's LidarPoint, 32 zero bytes otherwise.
 * lsa_dense_map_compare_*: one label per point, the ray from its origin to the point with extend = the tolerance (finite, >=
 * 0): 0 NOT_JUDGED (no ray, or len > max_range), 2 UNMAPPED (no hit), 3 THROUGH_MAP (hit whose t_out * tt < len - tolerance),
 * 1 CONSISTENT (any other hit); counts[4] the number of each.  _compare_frame: the context's current frame under the poses of
 * lsa_dense_map_carve_frame -- the labels of _compare_points of lsa_transform_frame_at's points and
 * lsa_transform_frame_origins_at's origins; returns the number of points (LSA_E_CAPACITY, nothing written, above capacity).
 * Two limits of a test by voxels: at tolerance 0 a point exactly on a voxel face may end its walk one voxel short (o + (t - o)
 * need not be t), and at grazing incidence the ray meets occupied voxels of the same surface well before the point, so far
 * ground reads THROUGH_MAP at a small tolerance; UNMAPPED is the robust label.
 * The calls wait for the insertions and carves in flight, change nothing in the map (no voxel, record, miss, "Rays", last
 * ordinal) and claim nothing in the table; a thread makes at most 3 * (4096 + 2) steps.  LSA_E_ARG, outputs and map untouched:
 * a NULL pointer, n < 0, n_origins neither 1 nor n, max_range not finite, not > 0 or above 4096 leaves, extend NaN (compare:
 * not finite or < 0), min_frames < 1, use_before neither 0 nor 1, reserved not 0.  n == 0 is LSA_OK.
 * lsa_dense_map_get_param: "CastRays" (rays cast by these calls since the last clear), "CastSeconds" (the host's, of the last).
 * lsa_scan_targets (host only): the rays of a spinning sensor at a pose: origin = the translation narrowed to float, target
 * (r, c) = the pose applied to (cos el_r cos az_c, cos el_r sin az_c, sin el_r), az_c = 2 pi c / n_azimuth, in double, narrowed
 * to float, ring-major.  A render is lsa_dense_map_cast of these with extend = +inf. */
typedef struct lsa_dense_cast_params_t
{
  double max_range;      /* metres, finite, > 0, at most 4096 leaves */
  double extend;         /* metres past the target; +inf: to max_range; NaN refused; compare: the tolerance, finite, >= 0 */
  double max_miss_ratio; /* the export's filter; below 0: none */
  int32_t min_frames;    /* >= 1 */
  int32_t use_before;    /* 0: every voxel; 1: only first_frame < before */
  int32_t before;
  int32_t reserved;      /* 0 */
} lsa_dense_cast_params_t;
typedef struct lsa_dense_hit_t
{
  uint64_t key;
  float entry, exit, depth;
  int32_t steps, source, status;
} lsa_dense_hit_t;
int lsa_dense_map_cast(lsa_dense_map* dm, const float* origins_xyz, int n_origins, const float* targets_xyz, int n, const lsa_dense_cast_params_t* params,
                       lsa_dense_hit_t* hits, lsa_point_t* points);
int lsa_dense_map_compare_points(lsa_dense_map* dm, const lsa_point_t* pts, int n, const float* origins_xyz, int n_origins, const lsa_dense_cast_params_t* params,
                                 uint8_t* labels, long long counts[4]);
int lsa_dense_map_compare_frame(lsa_dense_map* dm, int interpolate, const double H0[16], const double H1[16], double t0, double t1, double time_offset,
                                const lsa_dense_cast_params_t* params, uint8_t* labels, int capacity, long long counts[4]);
int lsa_scan_targets(const double pose16[16], const double* elevations_rad, int n_rings, int n_azimuth, float* origin_xyz, float* targets_xyz);
/* The pipeline's map under these calls; LSA_E_STATE while "DenseMap" is 0; each waits for the maps' work in flight and adds
 * nothing to a frame.  _render_dense_map_scan: lsa_dense_map_cast of lsa_scan_targets at pose16 (NULL: Tworld *
 * BaseToLidarOffset) with the params as given (extend = +inf for a scan); hits: n_rings * n_azimuth.
 * _compare_frame_to_dense_map: one label per point of lsa_slam_get_registered_frame, in its order, every device frame of the
 * last call under the poses the insertion used; returns their number.  params NULL: max_range 30, tolerance one leaf,
 * min_frames 1, ratio -1, use_before 2.  use_before == 2 (this call only): when the call that brought the current frame was
 * inserted into the map, before = that call's ordinal -- the map as it stood before this frame --, otherwise every voxel. */
int lsa_slam_cast_dense_map_rays(lsa_slam* s, const float* origins_xyz, int n_origins, const float* targets_xyz, int n, const lsa_dense_cast_params_t* params,
                                 lsa_dense_hit_t* hits, lsa_point_t* points);
int lsa_slam_render_dense_map_scan(lsa_slam* s, const double* pose16, const double* elevations_rad, int n_rings, int n_azimuth, const lsa_dense_cast_params_t* params,
                                   lsa_dense_hit_t* hits);
int lsa_slam_compare_frame_to_dense_map(lsa_slam* s, const lsa_dense_cast_params_t* params, uint8_t* labels, int capacity, long long counts[4]);

/* ------------------------------------------------------------------------- */
/* The keypoint log (Slam::LogKeypoints, slam_lib/src/Slam.cxx:1225-1255) in the memory of the device, and its replay under
 * a corrected trajectory (the part of Slam::RunPoseGraphOptimization that comes after the optimizer, Slam.cxx:416-475).
 * A frame of the log is the three RAW keypoint sets (BASE coordinates, not undistorted) of one logged pose.  Storage:
 * chunks of 32 MiB; a frame never straddles two, so growth never copies; a chunk whose frames have all been popped is
 * reused; nothing is freed while work may be in flight (lsa_collect_garbage).  The log is made by the first append: a
 * context that never logs allocates, enqueues and reads nothing for it.
 * Slam::LoggingStorage (PointCloudStorageType: PCL_CLOUD, OCTREE_COMPRESSED, PCD_ASCII, PCD_BINARY, PCD_BINARY_COMPRESSED)
 * is accepted by lsa_slam_set_param("LoggingStorage") and all five values mean the same thing here: uncompressed
 * LidarPoints in HBM (32 B a keypoint; about 1 MB per VLS-128 frame).  Nothing is compressed.
 * - lsa_kplog_append: a frame from LSA_SET_RAW_CURRENT, one device-to-device launch on the context's stream.
 * - lsa_kplog_append_points: a frame of the caller's own keypoints (pts[k] may be NULL where n[k] == 0).
 * - lsa_kplog_pop_front / _clear: drop the oldest frame / everything (_clear also ends a stop, see below).
 * - lsa_kplog_size: frames; lsa_kplog_count(frame, type): keypoints; lsa_kplog_get: copies them out, returns the number
 *   written; lsa_kplog_bytes: bytes of device memory held by the chunks.
 * When a chunk cannot be allocated the append fails with LSA_E_HIP (lsa_last_error says so), lsa_kplog_stopped turns 1 and
 * appends and replays answer LSA_E_STATE until lsa_kplog_clear.
 * - lsa_kplog_replay: ONE launch (k_log_replay) for all n = lsa_kplog_size frames and the types in type_mask, a thread per
 *   logged point: frame i >= 1 with undistort != 0 is moved by LinearTransformInterpolator(pose[i-1], pose[i]) with
 *   SetTimes(times[i] - times[i-1], 0.) evaluated at each point's own time, as the reference writes it (Slam.cxx:426-440);
 *   frame 0, and every frame with undistort == 0, by the rigid pose[i].  The per-point arithmetic is lsa_undistort's /
 *   lsa_stage_transformed's.  poses: n row-major 4x4.  The result -- frames ascending, inside a frame the logged order --
 *   is written into pinned host memory of the context (lsa_kplog_replayed returns it and its size; valid until the next
 *   replay) and copied to out[k] where out and out[k] are not NULL.  last_min / last_max [type][xyz]: the box of the LAST
 *   frame's moved keypoints (Slam.cxx:472-473); FLT_MAX / -FLT_MAX for a type without keypoints in it.
 *   LSA_E_ARG unless n == lsa_kplog_size and n >= 2.
 * - lsa_kplog_replay_to_grids: the same straight into the batch buffers of the device maps grids[k] (types in type_mask),
 *   followed by RollingGrid::Add(aggregate, fixed = false, time = -1, roll = false) on each (Slam.cxx:474); the caller
 *   rolls (lsa_device_grid_roll(grids[k], last_min[k], last_max[k]), Slam.cxx:475).
 * - lsa_kplog_replay_range: ONE launch (k_log_replay_range) for the frames first..last (inclusive) alone -- their tables, their
 *   points: a range costs what its points cost, not what the log costs.  poses / times are still those of all n =
 *   lsa_kplog_size frames (frame `first` >= 1 interpolates from pose[first - 1]); the caller may pass any poses.  rule:
 *     0  every frame by the rigid pose[i];
 *     1  the rebuild's rule, lsa_kplog_replay's with undistort != 0: SetTimes(times[i] - times[i-1], 0.);
 *     2  the sweep rule: SetTimes(-(times[i] - times[i-1]), 0.) -- pose[i-1] one sweep BEFORE pose[i], which is where the
 *        points of a frame whose times lie in [-sweep, 0] were taken; the geometry a registration wants.
 *   Frame 0 is rigid under every rule; the per-point arithmetic is lsa_kplog_replay's.  The result goes where lsa_kplog_replay's
 *   goes (lsa_kplog_replayed; out[k] where given).  box_min / box_max [type][xyz]: the box of ALL replayed points of a type;
 *   a NaN coordinate takes no part; FLT_MAX / -FLT_MAX for a type without points.
 *   LSA_E_ARG (nothing written) for a bad range or rule or n != lsa_kplog_size, LSA_E_STATE for a stopped log.
 * The descriptor store (lsa_place.hip; lsa_place_params_t and the descriptor: "Place recognition" above): a slot of
 * rings * sectors + sectors floats per logged frame, owned by the log, filled lazily.  It follows _append, _pop_front and
 * _clear; a change of any parameter invalidates all of it; poses are no part of it.
 * - lsa_kplog_describe(params, first, last): describes the frames of the range that have no valid descriptor (ONE launch of
 *   k_log_describe).  Returns how many it described.
 * - lsa_kplog_descriptors(first, last, out): copies the range's descriptors out, (last - first + 1) x (rings * sectors +
 *   sectors) floats; LSA_E_STATE when one of them has not been described.  lsa_kplog_descriptor_length: the floats of one
 *   under the parameters the store holds now (0: none yet).
 * - lsa_kplog_place_search(params, query, first, last, distance_out, shift_out): describes what is missing among `query`
 *   and first..last, ONE launch of k_place_search, ONE copy of the table (last - first + 1 entries) to pinned memory.
 * - lsa_kplog_described: how many frames the last of these calls described (a test's view of the laziness).
 * The three: LSA_E_STATE for a stopped log, LSA_E_ARG for a bad range, a query outside the log or parameters out of
 * limits, with nothing written.  lsa_debug_set "place_max_blocks" n: at most n workgroups a search launch (<= 0: the default). */
int lsa_kplog_describe(lsa_ctx* ctx, const lsa_place_params_t* params, int first, int last);
int lsa_kplog_descriptors(lsa_ctx* ctx, int first, int last, float* out);
int lsa_kplog_place_search(lsa_ctx* ctx, const lsa_place_params_t* params, int query, int first, int last, float* distance_out, int32_t* shift_out);
int lsa_kplog_described(const lsa_ctx* ctx);
int lsa_kplog_descriptor_length(const lsa_ctx* ctx);
/* Loop detection over the log (lsa_place_detect.hip; the definition: "Loop detection over the whole log" above).
 * - lsa_kplog_place_search_rows(params, first_query, last_query, query_stride, distance_out, shift_out): k_place_search_rows
 *   alone, no gates: the ragged table of the query set, row of query q = (distance, shift) of q against the frames 0..q-1,
 *   rows concatenated in the queries' order (a query 0 has an empty row).  Each entry equals lsa_place_distance_host.
 * - lsa_kplog_detect_loops(detect, poses17, n, out, capacity): n = lsa_kplog_size rows of 17 doubles; describes what is
 *   missing, then per run of consecutive queries whose tables fit the table's byte budget ONE launch of k_place_search_rows
 *   (the pairs behind the min_travelled and max_distance gates are not computed) and ONE of k_place_select_rows; the
 *   candidates accumulate on the device; ONE copy to pinned memory and ONE wait for the call.  Returns their number.
 * The table is scratch space of the context, 8 bytes a pair, at most 256 MiB (or one row, if that is larger); lsa_debug_set
 * "place_table_bytes" n lowers the budget to n bytes (<= 0: the default); "place_max_blocks" holds for both launches;
 * "place_untiled" 1 makes the search walk its columns one at a time instead of four (the same table; kept to measure against).
 * Refusals as above, with nothing written. */
int lsa_kplog_place_search_rows(lsa_ctx* ctx, const lsa_place_params_t* params, int first_query, int last_query, int query_stride, float* distance_out,
                                int32_t* shift_out);
int lsa_kplog_detect_loops(lsa_ctx* ctx, const lsa_loop_detect_t* detect, const double* poses17, int n, lsa_loop_candidate_t* out, int capacity);
int lsa_kplog_append(lsa_ctx* ctx);
int lsa_kplog_append_points(lsa_ctx* ctx, const lsa_point_t* const pts[3], const int n[3]);
int lsa_kplog_pop_front(lsa_ctx* ctx);
int lsa_kplog_clear(lsa_ctx* ctx);
int lsa_kplog_size(const lsa_ctx* ctx);
int lsa_kplog_count(const lsa_ctx* ctx, int frame, int type);
int lsa_kplog_get(lsa_ctx* ctx, int frame, int type, lsa_point_t* out, int capacity);
unsigned long long lsa_kplog_bytes(const lsa_ctx* ctx);
int lsa_kplog_stopped(const lsa_ctx* ctx);
int lsa_kplog_replay(lsa_ctx* ctx, unsigned type_mask, const double* poses, const double* times, int n, int undistort, lsa_point_t* const out[3],
                     float last_min[3][3], float last_max[3][3]);
long long lsa_kplog_replayed(const lsa_ctx* ctx, int type, const lsa_point_t** pts);
int lsa_kplog_replay_to_grids(lsa_ctx* ctx, unsigned type_mask, const double* poses, const double* times, int n, int undistort, lsa_device_grid* const grids[3],
                              float last_min[3][3], float last_max[3][3]);
int lsa_kplog_replay_range(lsa_ctx* ctx, unsigned type_mask, const double* poses, const double* times, int n, int first, int last, int rule,
                           lsa_point_t* const out[3], float box_min[3][3], float box_max[3][3]);

/* ------------------------------------------------------------------------- */
/* The table of map descriptors (lsa_map_place.hip; the definition: "Place recognition against the MAPS" above).  The context
 * owns ONE table of V + 1 slots of rings * sectors + sectors floats: slot i < V is the descriptor of the maps at viewpoint i,
 * slot V the query.  The source of the map points is "two float4 per point, n points" -- a device grid's own array of voxel
 * points, or an uploaded lsa_point_t array --, cut into contiguous slices ("map_describe_slice" points each, default 4096):
 *   k_map_slice_boxes  a workgroup per slice: its xy box (a NaN takes no part); once per map version
 *   k_map_describe     a workgroup of 256 per viewpoint and row of slices (blockIdx.y strides the slices): an LDS image of the
 *                      cells in the order-preserving coding of floats, LDS atomic max per point, then its non-empty words
 *                      merged into the viewpoint's zeroed image in global memory by 32-bit integer atomic max.  A slice whose
 *                      box lies farther from v than max_range * (1 + 2^-20) is passed over ("map_describe_cull" 0 switches
 *                      that off); a point whose squared planar distance exceeds that reach squared is dropped before the
 *                      square root and the angle.  Maxima commute: the bytes do not depend on the slicing or the cull.
 *   k_map_finish       a workgroup per viewpoint: decodes, writes the cells and the column norms, rings ascending
 * No float atomics; no workgroup waits for another.  The grids are read on their own stream behind their last modification,
 * as lsa_device_grid_get reads them; the call returns when the table is written.
 * - lsa_map_place_describe_points(params, pts, n, viewpoints, V): uploads the points and describes them; returns V.
 * - lsa_map_place_describe_grids(grids, params, viewpoints, V): grids[k] (NULL allowed) of the types in type_mask, all of
 *   this context.  The table is kept: when the parameters, the viewpoints (by content) and every used grid's modification
 *   count are those of the table, nothing is launched and 0 is returned; otherwise V.
 * - lsa_map_place_descriptors(first, last, out): copies slots first..last out (slot V only after a search described it).
 * - lsa_map_place_search(params, set, distance_out, shift_out): describes the keypoint set `set` (types of type_mask) into
 *   slot V with k_log_describe's code, ONE launch of k_place_search over the V viewpoints, ONE copy of the V (distance,
 *   shift) pairs to pinned memory, one wait.
 * - lsa_map_place_slices(boxes, capacity): the slices of the last description and (where boxes != NULL) their boxes, four
 *   floats each (min x, min y, max x, max y); returns the number of slices.  lsa_map_place_viewpoints: V of the table (0: none).
 * Refusals write nothing: LSA_E_ARG for parameters out of limits, V < 1, a viewpoint that is not finite, grids of another
 * context, a bad range; LSA_E_STATE for no table, a table made under other parameters, or an empty query set. */
int lsa_map_place_describe_points(lsa_ctx* ctx, const lsa_place_params_t* params, const lsa_point_t* pts, int n, const double* viewpoints, int V);
int lsa_map_place_describe_grids(lsa_ctx* ctx, lsa_device_grid* const grids[3], const lsa_place_params_t* params, const double* viewpoints, int V);
int lsa_map_place_descriptors(lsa_ctx* ctx, int first, int last, float* out);
int lsa_map_place_search(lsa_ctx* ctx, const lsa_place_params_t* params, int set, float* distance_out, int32_t* shift_out);
int lsa_map_place_slices(lsa_ctx* ctx, float* boxes, int capacity);
int lsa_map_place_viewpoints(const lsa_ctx* ctx);

/* ------------------------------------------------------------------------- */
/* Pose-graph optimization of relative-pose edges: the odometry chain of a logged trajectory plus the loop-closure edges
 * lsa_slam_register_logged_frames produces.  The whole definition -- retraction t += R rho, R = R Exp(phi); the error
 * e = [Rz^T (Ri^T (tj - ti) - tz) ; Log(Rz^T Ri^T Rj)]; its exact Jacobians; the order of every sum; the rules for small angles
 * and angles near pi; the Levenberg-Marquardt loop with a preconditioned conjugate gradient inside -- is
 * lidarslam_amd/csrc/lsa_pose_graph.h, compiled for the host and the device alike.  Plain least squares in these calls; robust losses on chosen
 * edges and on the priors, with a verdict per constraint: the lsa_pgo_*_robust calls further down.  Position
 * priors (GPS fixes) and the reference's RunPoseGraphOptimization on top of them: the next comment.
 * - lsa_pgo_edge_t: from -> to, `relative` the measured inv(P[from]) * P[to] (row-major 4x4), `information` its 6x6 weight
 *   over (translation, rotation) in the tangent of the retraction, row-major.  from != to.
 * - fixed[n]: non-zero = the pose is held.  At least one pose must be fixed (or, in the calls with priors, a prior given) and
 *   every free pose needs an edge; an index out of range, from == to or a non-finite entry: all LSA_E_ARG, nothing written.
 * - lsa_pgo_params_init: max_iterations 50, pcg_max_iter 500, pcg_tolerance 1e-8, initial_lambda 1e-6, lambda_shrink 0.25,
 *   lambda_grow 8, lambda_min 1e-12, lambda_max 1e12, gradient_tolerance 1e-12, step_tolerance 1e-10, cost_tolerance 1e-13,
 *   preconditioner 0 (block tridiagonal; 1 = its diagonal blocks alone, a knob for measurements), apply 0,
 *   odometry_information 0, odometry_sigma {0.05 m x 3, 0.01 rad x 3}.
 * - lsa_pgo_result_t.termination: LSA_PGO_* below; `message` names it (a static string).
 * - lsa_pgo_solve_host: the host statement, no device (ctx-free).  lsa_pgo_solve: the device solver (lsa_pose_graph.hip):
 *   k_pgo_linearize (a thread per edge), k_pgo_assemble (a thread per pose), a block parallel cyclic reduction of the
 *   tridiagonal preconditioner (ceil(log2 n) launches per factorization and per application, alpha / gamma of every level
 *   kept: LSA_E_CAPACITY above 262144 poses), k_pgo_spmv, two-level fixed-order dot products, no floating-point atomics: two
 *   runs give the same bits.  The host drives LM and PCG and reads one small status block per PCG iteration; alpha and beta
 *   stay on the device.  poses_out may be poses.  A refusal writes nothing.
 * - seams (one call each: copies plus the kernel named, or its host twin): lsa_pgo_linearize[_host] -> e[6 m], blocks[120 m]
 *   (Haa Hab Hbb ga gb per edge), chi2[m]; lsa_pgo_assemble[_host] at lambda -> D[36 n] (damped), g[6 n], L[36 n] = block
 *   (i, i-1), U[36 n] = block (i, i+1); lsa_pgo_tridiagonal_solve[_host] (device: cyclic reduction; host: block Thomas):
 *   returns 1 and leaves x untouched when a block is not positive definite; lsa_pgo_spmv[_host]: q = H_lambda p with the
 *   blocks beyond the chain.
 *   lsa_pgo_retract[_host]: out[i] = the retraction of pose i by delta[6 i .. 6 i + 5] (k_pgo_retract / its host twin);
 *   lsa_pgo_edge_jacobians_host: e[6], A[36], B[36] of ONE edge (row-major 6x6), host only -- the device's are held through the
 *   block records, which are made of them.
 * - lsa_pgo_information_from_covariance: the inverse of a symmetric positive definite 6x6 (host); LSA_E_ARG otherwise.
 * - lsa_slam_optimize_logged_trajectory(loop_edges, m, params, poses17_out, capacity, result): the graph of the logged
 *   trajectory.  Vertices: the n logged poses, pose 0 fixed.  Odometry edge i-1 -> i: Z = inv(P[i-1]) * P[i], information by
 *   params->odometry_information: 0 (the default, a choice: it works in "TwoDMode" and for a log whose covariances were
 *   popped) = diag(1 / odometry_sigma^2), default sigma 0.05 m and 0.01 rad, a choice too; 1 = the reference's rule
 *   (PoseGraphOptimization.cxx:237-244), the inverse of logged covariance i, LSA_E_ARG naming the frame when that is not
 *   positive definite.  loop_edges: from = revisited, to = query, relative = lsa_loop_closure_result_t.relative, information
 *   e.g. lsa_pgo_information_from_covariance(its covariance).  That a covariance over (X, Y, Z, rX, rY, rZ) serves as the
 *   information of this tangent (translation in the body frame, rotation vector) is the reference's own simplification.
 *   Writes n rows of 17 doubles as lsa_slam_get_trajectory gives them (capacity >= n rows) and returns n.  With
 *   params->apply != 0 the result goes straight into lsa_slam_set_trajectory_and_rebuild_maps; with 0 nothing the frame path
 *   reads is touched.  Waits for the map workers (an offline call); runs lsa_pgo_solve on the handle's scratch context.
 *   LSA_E_STATE when "LoggingTimeout" is 0, keypoint logging stopped or the keypoint log does not cover the logged poses
 *   (mode 1: or the covariance log does not); LSA_E_ARG for fewer than two poses, an edge outside the log or bad parameters;
 *   nothing changed.  Read-only parameter "PoseGraphSeconds": the last call's solve by the host's clock. */
#define LSA_PGO_MAX_ITERATIONS 0
#define LSA_PGO_GRADIENT 1
#define LSA_PGO_STEP 2
#define LSA_PGO_COST 3
#define LSA_PGO_LAMBDA_CEILING 4
#define LSA_PGO_LINEAR_SOLVER_FAILED 5
typedef struct lsa_pgo_edge_t
{
  int32_t from, to;
  double relative[16];
  double information[36];
} lsa_pgo_edge_t;
typedef struct lsa_pgo_params_t
{
  int32_t max_iterations;
  int32_t pcg_max_iter;
  int32_t preconditioner;
  int32_t apply;                /* lsa_slam_optimize_logged_trajectory: hand the result to ..._set_trajectory_and_rebuild_maps */
  int32_t odometry_information; /* lsa_slam_optimize_logged_trajectory: 0 diag(1 / odometry_sigma^2), 1 inverse logged covariance */
  int32_t reserved;
  double pcg_tolerance;
  double initial_lambda, lambda_shrink, lambda_grow, lambda_min, lambda_max;
  double gradient_tolerance, step_tolerance, cost_tolerance;
  double odometry_sigma[6];
} lsa_pgo_params_t;
typedef struct lsa_pgo_result_t
{
  double initial_cost, final_cost; /* F = 1/2 sum chi2 */
  double largest_step;             /* the largest max |delta| of an accepted step */
  double final_lambda;
  int32_t iterations, accepted_steps, rejected_steps;
  int32_t pcg_iterations, last_pcg_iterations, pcg_truncated;
  int32_t termination, reserved;
  const char* message;
} lsa_pgo_result_t;
/* Position priors in the pose graph.
 * - lsa_pgo_prior_t: the measured `position` of a point carried by pose `pose`, `information` its 3x3 weight (row-major).  All
 *   priors of a solve share offset16 = (Ro, to), a row-major 4x4 (may be NULL when k is 0): d = Ri^T (g - ti),
 *   e = Ro^T (d - to), A = de/ddelta_i = [-Ro^T, Ro^T [d]x].  For GPS fixes offset16 = inverse(gpsToSensor), as the reference
 *   sets it.  A graph needs a fixed pose or a prior; every free pose still needs an edge; a prior on a fixed pose counts in the
 *   cost alone; an index out of range, a non-finite entry or k < 0: LSA_E_ARG, nothing written.  The cost is 1/2 sum chi2 over
 *   the m edge values followed by the k prior values.
 * - lsa_pgo_solve_priors[_host], lsa_pgo_assemble_priors[_host], lsa_pgo_spmv_priors[_host]: the calls above with priors; with
 *   k = 0 they are those calls, bit for bit (which are now their k = 0 case).  lsa_pgo_linearize_priors[_host] -> e[3 k],
 *   blocks[42 k] (Haa[36] ga[6] per prior), chi2[k] (k_pgo_linearize_priors / its host twin).  lsa_pgo_prior_jacobian_host:
 *   e[3], A[18] (3x6 row-major) of ONE prior.  lsa_pgo_premultiply[_host]: out[i] = W * P[i]; lsa_pgo_reanchor[_host]:
 *   out[i] = inv(P[0]) * P[i] (k_pgo_premultiply, k_pgo_reanchor / their host twins; poses_out may be poses16).
 * - lsa_pgo_information_from_covariance3: the inverse of a symmetric positive definite 3x3 (host); LSA_E_ARG otherwise.
 * - lsa_gps_match_trajectory (host): per GPS fix, in order, match_out[f] = the index of the logged pose, dated
 *   slam_times[j] + time_offset, nearest in time to gps_times[f] within max_time_diff (inclusive; the reference uses 0.1 s), the
 *   earlier of two equally near; -1 when there is none, and for a fix whose pose is the pose of the fix accepted before it.
 *   Times finite and ascending, else LSA_E_ARG.
 * - lsa_trajectory_alignment (host): the rigid T (row-major 4x4) minimising sum |T from_i - to_i|^2 over `pairs` pairs of
 *   points (xyz each), Horn's closed form; for fewer than three pairs, or when the two largest eigenvalues of Horn's matrix are
 *   within 1e-9 of the largest (collinear tracks), x -> R x + (to_0 - from_0) with R the least rotation carrying the chord
 *   from_last - from_0 onto to_last - to_0 (the identity when a chord vanishes).
 * - lsa_slam_run_pose_graph_optimization(gps_times, gps_xyz, gps_cov9, G, gps_to_sensor16, time_offset, params, poses17_out,
 *   capacity, result): Slam::RunPoseGraphOptimization.  Fixes are matched to the logged poses (above, 0.1 s); W = the alignment
 *   of the matched antenna positions (P_i * inverse(gps_to_sensor)).t onto their fixes; the graph: the logged poses premultiplied
 *   by W, all free, the odometry chain as lsa_slam_optimize_logged_trajectory builds it (params->odometry_information), a prior
 *   per matched fix with the inverse of its covariance; solved by lsa_pgo_solve_priors on the handle's scratch context.  Out:
 *   gps_to_sensor16 = the optimized pose 0 (in the GPS frame), rows i = inv(opt[0]) * opt[i] with the logged times; returns n.
 *   params->apply as above.  LSA_E_STATE as lsa_slam_optimize_logged_trajectory; LSA_E_ARG, the text naming the case, for fewer
 *   than two logged poses or fixes, time intervals that do not overlap (closed intervals, logged times + time_offset), no fix
 *   matched, a covariance that is not positive definite (the fix is named), bad parameters; nothing changed.
 *   "PoseGraphSeconds" is updated. */
typedef struct lsa_pgo_prior_t
{
  int32_t pose, reserved;
  double position[3];
  double information[9];
} lsa_pgo_prior_t;
void lsa_pgo_params_init(lsa_pgo_params_t* params);
int lsa_pgo_solve_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_params_t* params, double* poses_out,
                       lsa_pgo_result_t* result);
int lsa_pgo_solve(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_params_t* params, double* poses_out,
                  lsa_pgo_result_t* result);
int lsa_pgo_linearize_host(const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, double* e_out, double* blocks_out, double* chi2_out);
int lsa_pgo_linearize(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, double* e_out, double* blocks_out, double* chi2_out);
int lsa_pgo_assemble_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, double* D_out, double* g_out,
                          double* L_out, double* U_out);
int lsa_pgo_assemble(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, double* D_out, double* g_out,
                     double* L_out, double* U_out);
int lsa_pgo_tridiagonal_solve_host(int n, const double* D, const double* L, const double* U, const double* b, double* x);
int lsa_pgo_tridiagonal_solve(lsa_ctx* ctx, int n, const double* D, const double* L, const double* U, const double* b, double* x);
int lsa_pgo_spmv_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, const double* p, double* q);
int lsa_pgo_spmv(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, double lambda, const double* p, double* q);
int lsa_pgo_retract_host(const double* poses16, int n, const double* delta, double* poses_out);
int lsa_pgo_retract(lsa_ctx* ctx, const double* poses16, int n, const double* delta, double* poses_out);
int lsa_pgo_edge_jacobians_host(const double* poses16, int n, const lsa_pgo_edge_t* edge, double* e6, double* A36, double* B36);
int lsa_pgo_information_from_covariance(const double* cov36, double* info36);
int lsa_slam_optimize_logged_trajectory(lsa_slam* s, const lsa_pgo_edge_t* loop_edges, int m, const lsa_pgo_params_t* params, double* poses17_out, int capacity,
                                        lsa_pgo_result_t* result);
int lsa_pgo_solve_priors_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                              const double* offset16, const lsa_pgo_params_t* params, double* poses_out, lsa_pgo_result_t* result);
int lsa_pgo_solve_priors(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                         const double* offset16, const lsa_pgo_params_t* params, double* poses_out, lsa_pgo_result_t* result);
int lsa_pgo_linearize_priors_host(const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, double* e_out, double* blocks_out,
                                  double* chi2_out);
int lsa_pgo_linearize_priors(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, double* e_out, double* blocks_out,
                             double* chi2_out);
int lsa_pgo_assemble_priors_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                                 const double* offset16, double lambda, double* D_out, double* g_out, double* L_out, double* U_out);
int lsa_pgo_assemble_priors(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                            const double* offset16, double lambda, double* D_out, double* g_out, double* L_out, double* U_out);
int lsa_pgo_spmv_priors_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                             const double* offset16, double lambda, const double* p, double* q);
int lsa_pgo_spmv_priors(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const lsa_pgo_prior_t* priors, int k,
                        const double* offset16, double lambda, const double* p, double* q);
int lsa_pgo_prior_jacobian_host(const double* poses16, int n, const lsa_pgo_prior_t* prior, const double* offset16, double* e3, double* A18);
int lsa_pgo_premultiply_host(const double* poses16, int n, const double* W16, double* poses_out);
int lsa_pgo_premultiply(lsa_ctx* ctx, const double* poses16, int n, const double* W16, double* poses_out);
int lsa_pgo_reanchor_host(const double* poses16, int n, double* poses_out);
int lsa_pgo_reanchor(lsa_ctx* ctx, const double* poses16, int n, double* poses_out);
int lsa_pgo_information_from_covariance3(const double* cov9, double* info9);
int lsa_gps_match_trajectory(const double* slam_times, int n, const double* gps_times, int G, double time_offset, double max_time_diff, int32_t* match_out);
int lsa_trajectory_alignment(const double* from_xyz, const double* to_xyz, int pairs, double* T16_out);
int lsa_slam_run_pose_graph_optimization(lsa_slam* s, const double* gps_times, const double* gps_xyz, const double* gps_cov9, int G, double* gps_to_sensor16,
                                         double time_offset, const lsa_pgo_params_t* params, double* poses17_out, int capacity, lsa_pgo_result_t* result);

/* Robust losses in the pose graph, and a verdict per constraint (the definition, with the order of every
 * operation, is the section ROBUST LOSS of lidarslam_amd/csrc/lsa_pose_graph.h).
 * - A loss acts on s = chi2 of one constraint with a scale c > 0 in sigmas: Huber, Geman-McClure or Tukey (LSA_PGO_LOSS_*),
 *   first-order IRLS (the weight w = rho'(s) multiplies the constraint's block record, no second-derivative term: g2o's rule),
 *   and the cost is F = 1/2 sum rho.  Geman-McClure and Tukey are not convex: the solve finds the minimum nearest its start.
 * - lsa_pgo_robust_t: edge_loss / edge_scale act on the edges edge_mask selects (m bytes, non-zero = robustified; NULL = every
 *   edge), prior_loss / prior_scale on every prior.  lsa_pgo_robust_init: both losses NONE, both scales 1.  A loss outside
 *   0..3, or a scale that is not finite and positive while its loss is not NONE: LSA_E_ARG, nothing written.  robust NULL = init.
 * - lsa_pgo_robust_rho_host(loss, scale, s, &rho, &w): the loss alone.
 * - lsa_pgo_linearize_robust[_host] -> e[6 m], blocks[120 m] (each record times its w), chi2[m] (raw), rho[m], w[m];
 *   lsa_pgo_linearize_robust_priors[_host] -> e[3 k], blocks[42 k], chi2[k], rho[k], w[k] (prior_loss on every prior).
 * - lsa_pgo_solve_robust[_host]: lsa_pgo_solve_priors[_host] under the losses (which is now its case of both losses NONE, bit
 *   for bit).  edge_verdict_out (2 m doubles) and prior_verdict_out (2 k doubles) may be NULL; else {chi2, weight} per
 *   constraint at the returned poses, weight 1 for a constraint that is not robustified (on the device: one more launch of the
 *   chi2 kernels after the loop, copied back with the poses).
 * - lsa_slam_optimize_logged_trajectory_robust: lsa_slam_optimize_logged_trajectory with edge_loss on the caller's loop edges
 *   alone (the odometry chain is never discounted: it keeps the graph connected); loop_verdict_out (2 m doubles or NULL).
 *   lsa_slam_run_pose_graph_optimization_robust: lsa_slam_run_pose_graph_optimization with prior_loss on the GPS priors;
 *   fix_verdict_out (2 G doubles or NULL): {chi2, weight} per fix, {0, -1} for a fix that matched no pose.  Refusals, `apply`,
 *   "PoseGraphSeconds" and the scratch context as in those calls, which forward here with robust = init. */
#define LSA_PGO_LOSS_NONE 0
#define LSA_PGO_LOSS_HUBER 1
#define LSA_PGO_LOSS_GEMAN_MCCLURE 2
#define LSA_PGO_LOSS_TUKEY 3
typedef struct lsa_pgo_robust_t
{
  int32_t edge_loss, prior_loss;
  double edge_scale, prior_scale;
} lsa_pgo_robust_t;
void lsa_pgo_robust_init(lsa_pgo_robust_t* robust);
int lsa_pgo_robust_rho_host(int loss, double scale, double s, double* rho_out, double* w_out);
int lsa_pgo_linearize_robust_host(const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask, const lsa_pgo_robust_t* robust, double* e_out,
                                  double* blocks_out, double* chi2_out, double* rho_out, double* w_out);
int lsa_pgo_linearize_robust(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask, const lsa_pgo_robust_t* robust,
                             double* e_out, double* blocks_out, double* chi2_out, double* rho_out, double* w_out);
int lsa_pgo_linearize_robust_priors_host(const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, const lsa_pgo_robust_t* robust,
                                         double* e_out, double* blocks_out, double* chi2_out, double* rho_out, double* w_out);
int lsa_pgo_linearize_robust_priors(lsa_ctx* ctx, const double* poses16, int n, const lsa_pgo_prior_t* priors, int k, const double* offset16, const lsa_pgo_robust_t* robust,
                                    double* e_out, double* blocks_out, double* chi2_out, double* rho_out, double* w_out);
int lsa_pgo_solve_robust_host(const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask, const lsa_pgo_prior_t* priors,
                              int k, const double* offset16, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust, double* poses_out, lsa_pgo_result_t* result,
                              double* edge_verdict_out, double* prior_verdict_out);
int lsa_pgo_solve_robust(lsa_ctx* ctx, const double* poses16, int n, const uint8_t* fixed, const lsa_pgo_edge_t* edges, int m, const uint8_t* edge_mask,
                         const lsa_pgo_prior_t* priors, int k, const double* offset16, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust, double* poses_out,
                         lsa_pgo_result_t* result, double* edge_verdict_out, double* prior_verdict_out);
int lsa_slam_optimize_logged_trajectory_robust(lsa_slam* s, const lsa_pgo_edge_t* loop_edges, int m, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust,
                                               double* poses17_out, int capacity, lsa_pgo_result_t* result, double* loop_verdict_out);
int lsa_slam_run_pose_graph_optimization_robust(lsa_slam* s, const double* gps_times, const double* gps_xyz, const double* gps_cov9, int G, double* gps_to_sensor16,
                                                double time_offset, const lsa_pgo_params_t* params, const lsa_pgo_robust_t* robust, double* poses17_out, int capacity,
                                                lsa_pgo_result_t* result, double* fix_verdict_out);

/* Close every loop of the log: detect, register, solve, apply -- exactly the composition of the calls above.
 *  1. lsa_slam_detect_loop_closures(detect).
 *  2. Every candidate in order: lsa_slam_register_logged_frames(query, frame, loop_params, P[frame] * Rz(yaw)), all under the
 *     logged poses as they stand.
 *  3. An edge {from = frame, to = query, relative = the registration's} with lsa_pgo_information_from_covariance where the
 *     registration's status is 0 and its covariance is positive definite.
 *  4. One lsa_slam_optimize_logged_trajectory_robust over these edges; pgo_params->apply decides whether its poses go through
 *     lsa_slam_set_trajectory_and_rebuild_maps.
 * Returns the number of reports (= candidates) written; poses17_out gets the n = lsa_slam_logged_frames optimized poses
 * (capacity >= n rows), *result the solver's summary, reports_out one lsa_loop_report_t per candidate: status = the
 * registration's (0 registered, 1 too few matches, < 0 the LSA_E_* code of a refused registration), edge = its index among
 * the loop edges or -1, {chi2, weight} its verdict at the returned poses ({0, -1} without an edge).  Without a candidate, or
 * without an edge, nothing is solved and nothing changes: the poses are the logged ones, result->iterations is 0 and
 * result->message says so.  NULL detect / loop_params / pgo_params / robust = their defaults.  Refusals as the calls it is
 * made of; report_capacity below queries * per_query is LSA_E_ARG. */
typedef struct lsa_loop_report_t
{
  int32_t query;
  int32_t frame;
  float distance;                 /* of the descriptors */
  int32_t status;
  double yaw;                     /* [rad] the start guess's turn */
  int32_t iterations;             /* of the registration's ICP loop */
  int32_t edge;
  double position_error;          /* [m] of the registration */
  double chi2;
  double weight;
} lsa_loop_report_t;
int lsa_slam_close_loops(lsa_slam* s, const lsa_loop_detect_t* detect, const lsa_loop_closure_params_t* loop_params, const lsa_pgo_params_t* pgo_params,
                         const lsa_pgo_robust_t* robust, double* poses17_out, int capacity, lsa_pgo_result_t* result, lsa_loop_report_t* reports_out,
                         int report_capacity);

/* ---- the rolling voxel map (host) ---------------------------
 * LidarSlam::RollingGrid -- slam_lib/include/LidarSlam/RollingGrid.h:63-212,
 * slam_lib/src/RollingGrid.cxx.  Map maintenance runs on host threads beside the
 * device work (once per keyframe); the handle below is the class the pipeline
 * uses, exposed so that a maintainer can swap it in on its own and so that the
 * tests can compare it with the oracle call by call (no GPU involved).
 * Parameter names: "GridSize", "VoxelResolution", "LeafSize",
 * "MinFramesPerVoxel", "Sampling" (0 FIRST .. 4 CENTROID), "DecayingThreshold", and "AddThreads" (host threads
 * Add uses on a big cloud; an implementation knob, the map is the same for any value). */
typedef struct lsa_rolling_grid lsa_rolling_grid;
lsa_rolling_grid* lsa_rolling_grid_create(void);
void lsa_rolling_grid_destroy(lsa_rolling_grid* g);
int lsa_rolling_grid_set(lsa_rolling_grid* g, const char* name, double value);
/* RollingGrid::Reset (position may be NULL), ::Clear, ::Size */
void lsa_rolling_grid_reset(lsa_rolling_grid* g, const float position[3]);
void lsa_rolling_grid_clear(lsa_rolling_grid* g);
int lsa_rolling_grid_size(const lsa_rolling_grid* g);
/* RollingGrid::Roll, ::Add (RollingGrid.cxx:117-318), ::ClearOldPoints */
void lsa_rolling_grid_roll(lsa_rolling_grid* g, const float min_point[3], const float max_point[3]);
int lsa_rolling_grid_add(lsa_rolling_grid* g, const lsa_point_t* pts, int n, int fixed, double current_time, int roll);
void lsa_rolling_grid_clear_old_points(lsa_rolling_grid* g, double current_time);
/* RollingGrid::Get(clean): returns the number of points written */
int lsa_rolling_grid_get(const lsa_rolling_grid* g, int clean, lsa_point_t* out, int capacity);
/* RollingGrid::BuildSubMapKdTree: whole map when min_point is NULL, else the
 * bounding-box overload (RollingGrid.cxx:363-442).  Returns the sub-map size. */
int lsa_rolling_grid_build_submap(lsa_rolling_grid* g, const float min_point[3], const float max_point[3], int min_nb_points);
/* IsSubMapKdTreeValid / GetSubMap */
int lsa_rolling_grid_submap_valid(const lsa_rolling_grid* g);
int lsa_rolling_grid_submap(const lsa_rolling_grid* g, lsa_point_t* out, int capacity);

/* ------------------------------------------------------------------------- */
/* PCD v0.7 files of LidarPoint clouds; host only, no GPU.  Written from the format's description (no PCL): header entries
 * VERSION FIELDS SIZE TYPE COUNT WIDTH HEIGHT VIEWPOINT POINTS DATA and # comments; DATA ascii, binary (packed records),
 * binary_compressed (two uint32 -- compressed size, raw size -- then an LZF stream of the columns, field after field).
 * Reading takes any field order, ignores fields a LidarPoint does not have, gives 0 to those the file does not have, and
 * converts types I / U / F of sizes 1, 2, 4, 8 as C++ converts them; only COUNT 1 fields are used, the others are skipped
 * by their width; w = 1.  Writing emits x y z time intensity laser_id device_id label (SIZE 4 4 4 8 4 2 1 1, TYPE F F F F
 * F U U U: 28-byte records); ascii values are printed so that they read back to the same bits.
 * format: 0 ascii, 1 binary, 2 binary_compressed (PCDFormat, PointCloudStorage.h:60-65).
 * - lsa_pcd_info: number of points and format.  lsa_pcd_read: returns the file's number of points, writes at most
 *   `capacity`.  Both: LSA_E_ARG for a malformed file, lsa_pcd_last_error() (of the calling thread) names file and line.
 * - lsa_pcd_write: 0; -3 and no file for an empty cloud, -4 for an unknown format (savePointCloudToPCD).
 * - lsa_lzf_compress / _decompress: the LZF stage on its own; *written = bytes produced (_compress: also when they do not
 *   fit, with LSA_E_CAPACITY); a malformed stream or one that outgrows `capacity` is LSA_E_ARG. */
int lsa_pcd_info(const char* path, int* n, int* format);
int lsa_pcd_read(const char* path, lsa_point_t* out, int capacity);
int lsa_pcd_write(const char* path, const lsa_point_t* pts, int n, int format);
const char* lsa_pcd_last_error(void);
int lsa_lzf_compress(const void* in, size_t n, void* out, size_t capacity, size_t* written);
int lsa_lzf_decompress(const void* in, size_t n, void* out, size_t capacity, size_t* written);

/* ------------------------------------------------------------------------- */
/* Synthetic spinning-LiDAR sequences; host only, no GPU.      */
/* model: 16 (VLP-16, 16x1800), 64 (HDL-64, 64x2048), 128 (VLS-128, 128x2048) */
int lsa_synth_sensor(int model, int* nrings, int* ncols, double* el_min_deg, double* el_max_deg);
/* Returns the number of points written, -1 unknown model, -2 capacity. */
int lsa_synth_frame(int model, uint64_t seed, int frame, lsa_point_t* out, int capacity, uint64_t* stamp_us);
/* Ground-truth BASE pose at the stamp of `frame` relative to frame 0. */
void lsa_synth_pose(int frame, double T[16]);

#ifdef __cplusplus
}
#endif
#endif /* LIDARSLAM_AMD_H */
