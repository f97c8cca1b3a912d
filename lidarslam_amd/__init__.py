"""lidarslam_amd -- MI355X-native scan-matching hot path of Perception4D/LidarSlam.

Python front-end (ctypes) of liblidarslam_amd.so.  Two levels, both thin:

* :class:`Context`  -- the kernel-level C ABI (include/lidarslam_amd.h): upload a scan, extract
  keypoints, set a kNN target, match, accumulate normal equations, undistort.
* :class:`Slam`     -- the pipeline: ``add_frame`` / ``world_transform`` mirror
  ``LidarSlam::Slam::AddFrame`` / ``GetWorldTransform`` (slam_lib/include/LidarSlam/Slam.h:111-146).

There is no CPU fallback: without the built library or without a HIP device every constructor
raises.  The CPU oracle under ``oracle/`` is test infrastructure and is never imported from here.
"""
from ._abi import (  # noqa: F401
    ABI_SYMBOLS,
    E_ARG,
    E_CAPACITY,
    E_HIP,
    E_NO_DEVICE,
    E_STATE,
    KNN_MAX,
    SIGNATURES,
    TARGET_MAP,
    TARGET_PREVIOUS,
    IcpLink,
    LsaError,
    SolveResult,
    lib,
)
from ._native import (  # noqa: F401
    BLOB,
    EDGE,
    LIB_PATH,
    MATCH_NSTATUS,
    PLANE,
    POINT_DTYPE,
    SET_RAW_CURRENT,
    SET_RAW_PREVIOUS,
    SET_WORKING,
    ExtractParams,
    KernelStat,
    MatchParams,
    pose16,
    ptr,
    synth_frame,
    synth_pose,
)
from ._context import *  # noqa: F401,F403
from ._dense_map import *  # noqa: F401,F403
from ._grids import *  # noqa: F401,F403
from ._pcd import *  # noqa: F401,F403
from ._place import *  # noqa: F401,F403
from ._pose_graph import *  # noqa: F401,F403
from ._sensors import *  # noqa: F401,F403
from ._slam import *  # noqa: F401,F403

__all__ = ["Context", "Slam", "ExtractParams", "MatchParams", "POINT_DTYPE", "lib", "LsaError", "read_pcd", "write_pcd"]
