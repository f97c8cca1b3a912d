"""examples/slam_place_recognition.cpp -- map forward and back with the keypoint log on, recognize the place of the last
frame, register it against the log around the best candidate from the guess pose[candidate] * Rz(yaw) -- through the C++
mirror gives what the same calls give through the Python front end (one C ABI).  Without a GPU the example compiles, links
and refuses to run."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_place_recognition")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_place_recognition")
    forward = 12
    r = subprocess.run([exe, "16", str(forward)], capture_output=True, text=True, check=True)
    lines = [line.split()[1:] for line in r.stdout.strip().splitlines() if line.startswith("#")]
    extra = {}
    for words in lines:
        extra.setdefault(words[0], []).append([float(v) for v in words[1:]])
    frames = [L.synth_frame(16, 1000, f) for f in range(forward)]
    period = frames[1][1] - frames[0][1]
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    for seq, c in enumerate(list(range(forward)) + list(range(forward - 2, -1, -1))):
        s.add_frame(frames[c][0], frames[0][1] + seq * period, seq)
    P, t, _ = s.trajectory()
    query = P.shape[0] - 1
    assert extra["query"] == [[query]]
    found = s.recognize_place(query, capacity=3, min_travelled=2.0, max_distance=0.0, exclusion_half_window=2)
    assert len(found) >= 1 and len(extra["candidate"]) == len(found)
    for (frame, distance, shift, yaw), printed in zip(found, extra["candidate"]):
        assert printed[0] == frame and printed[2] == shift and printed[3] == yaw  # %.17g gives the double back
        assert np.float32(printed[1]) == distance                               # %.9g the float
    frame, _, _, yaw = found[0]
    assert frame <= 1  # the last frame is the first cloud again
    Rz = np.eye(4)
    Rz[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    reg = s.register_logged_frames(query, frame, L.LoopClosureParams(revisited_half_window=2), P[frame] @ Rz)
    assert extra["registered"] == [[reg.status, reg.iterations]] and reg.status == 0
    assert np.allclose(extra["relative"][0], reg.relative[:3, 3], atol=1e-9, rtol=0)
    assert np.allclose(extra["errors"][0], [reg.position_error, reg.orientation_error], atol=1e-8, rtol=0)
    s.close()
