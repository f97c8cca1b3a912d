"""examples/slam_gps_pose_graph.cpp -- map forward and back with the keypoint log on, make a GPS track from a known world
transform, RunPoseGraphOptimization, add two more frames -- through the C++ mirror gives what the same calls give through the
Python front end (one C ABI).  Without a GPU the example compiles, links and refuses to run."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_gps_pose_graph")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


def xyzrpy(x, y, z, rx, ry, rz):
    """LidarSlam::Transform(x, y, z, rx, ry, rz): R = Rz Ry Rx"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return np.array([[cy * cz, sx * sy * cz - cx * sz, cx * sy * cz + sx * sz, x], [cy * sz, sx * sy * sz + cx * cz, cx * sy * sz - sx * cz, y],
                     [-sy, sx * cy, cx * cy, z], [0.0, 0.0, 0.0, 1.0]])


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_gps_pose_graph")
    forward = 12
    r = subprocess.run([exe, "16", str(forward)], capture_output=True, text=True, check=True)
    extra = {}
    for line in r.stdout.strip().splitlines():
        if line.startswith("#"):
            words = line.split()[1:]
            extra.setdefault(words[0], []).append([float(v) for v in words[1:]])
    frames = [L.synth_frame(16, 1000, f) for f in range(forward)]
    period = frames[1][1] - frames[0][1]
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    order = list(range(forward)) + list(range(forward - 2, -1, -1))
    for seq, c in enumerate(order):
        s.add_frame(frames[c][0], frames[0][1] + seq * period, seq)
    P, t, _ = s.trajectory()
    n = P.shape[0]
    world, antenna = xyzrpy(100.0, -50.0, 10.0, 0.02, -0.03, 0.8), xyzrpy(0.4, -0.3, 1.2, 0.1, -0.2, 0.3)
    g = np.array([(world @ P[i] @ antenna)[:3, 3] for i in range(n)])
    g += 0.2 * np.sin(np.pi * np.arange(n) / (n - 1))[:, None] * np.array([0.0, 0.8, 0.6])
    got, _, cal, res, matches = s.run_pose_graph_optimization(t, g, np.repeat(np.eye(3)[None] * 9e-4, n, 0), gps_to_sensor=np.linalg.inv(antenna), apply=True)
    assert extra["gps"] == [[n]] and list(matches) == list(range(n))
    assert extra["solve"] == [[res.termination, res.iterations, res.pcg_iterations]]
    assert np.allclose(extra["cost"][0], [res.initial_cost, res.final_cost], rtol=1e-8, atol=0)
    assert np.allclose(extra["last"][0], got[-1][:3, 3], atol=1e-9, rtol=0)
    assert np.allclose(extra["calibration"][0], cal[:3, 3], atol=1e-9, rtol=0)
    for k in range(2):
        s.add_frame(frames[1 + k][0], frames[0][1] + (len(order) + k) * period, len(order) + k)
        assert np.allclose(extra["frame"][k], s.world_transform()[:3, 3], atol=1e-9, rtol=0)
    s.close()
