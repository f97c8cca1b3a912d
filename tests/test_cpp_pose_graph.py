"""examples/slam_pose_graph.cpp -- map forward and back with the keypoint log on, recognize the place of the last frame, register
it, optimize the logged trajectory with that edge on the device and rebuild the maps, add two more frames -- through the C++
mirror gives what the same calls give through the Python front end (one C ABI).  Without a GPU the example compiles, links and
refuses to run."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_pose_graph")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_pose_graph")
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
    query = P.shape[0] - 1
    frame, _, _, yaw = s.recognize_place(query, capacity=3, min_travelled=2.0, max_distance=0.0, exclusion_half_window=2)[0]
    Rz = np.eye(4)
    Rz[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    reg = s.register_logged_frames(query, frame, L.LoopClosureParams(revisited_half_window=2), P[frame] @ Rz)
    assert reg.status == 0 and extra["edge"] == [[frame, query]]
    got, _, res = s.optimize_trajectory([(frame, query, reg.relative, L.information_from_covariance(reg.covariance))], apply=True)
    assert extra["solve"] == [[res.termination, res.iterations, res.pcg_iterations]]
    assert np.allclose(extra["cost"][0], [res.initial_cost, res.final_cost], rtol=1e-8, atol=0)
    assert np.allclose(extra["last"][0], got[-1][:3, 3], atol=1e-9, rtol=0)
    for k in range(2):
        s.add_frame(frames[1 + k][0], frames[0][1] + (len(order) + k) * period, len(order) + k)
        assert np.allclose(extra["frame"][k], s.world_transform()[:3, 3], atol=1e-9, rtol=0)
    s.close()
