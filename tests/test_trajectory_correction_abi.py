"""CPU side of the keypoint log and the trajectory correction: every new lsa_* entry is declared in the header, exported
by the library and bound; examples/slam_trajectory_correction.cpp compiles and links against the C++ mirror."""
import re
import subprocess

from test_abi import ROOT, declared_functions
from test_cpp_api import build_example

NEW = [
    "lsa_kplog_append", "lsa_kplog_append_points", "lsa_kplog_pop_front", "lsa_kplog_clear", "lsa_kplog_size", "lsa_kplog_count", "lsa_kplog_get",
    "lsa_kplog_bytes", "lsa_kplog_replay", "lsa_slam_set_trajectory_and_rebuild_maps", "lsa_slam_logged_frames", "lsa_slam_get_logged_keypoints",
]


def test_new_entries_are_declared_exported_and_bound(L):
    lib, declared = L.lib(), declared_functions()
    for name in NEW:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in L.ABI_SYMBOLS, name
    for method in ("logged_frames", "logged_keypoints", "set_trajectory"):
        assert callable(getattr(L.Slam, method))
    for method in ("kplog_append", "kplog_append_points", "kplog_pop_front", "kplog_clear", "kplog_size", "kplog_count", "kplog_get", "kplog_bytes", "kplog_replay"):
        assert callable(getattr(L.Context, method))


def test_the_mirror_carries_the_calls_and_no_stale_claim():
    src = open(f"{ROOT}/lidarslam_amd/include/LidarSlam/Slam.h").read()
    assert re.search(r"void SetTrajectoryAndRebuildMaps\(const std::vector<Transform>&", src)
    assert re.search(r"PointCloud::Ptr GetLoggedKeypoints\(Keypoint k, std::size_t frame\)", src)
    head = src[: src.index("#pragma once")]
    assert "not supported on this build" not in head  # (it listed PCD map IO and the sensor constraints, which are built)


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_trajectory_correction")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr
