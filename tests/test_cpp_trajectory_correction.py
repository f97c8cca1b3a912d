"""examples/slam_trajectory_correction.cpp -- map with the keypoint log on, bend the trajectory, SetTrajectoryAndRebuildMaps,
two more frames -- through the C++ mirror gives what the same calls give through the Python front end (one C ABI)."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example
from test_gpu_trajectory_correction import bend


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_trajectory_correction")
    mapped = 6
    r = subprocess.run([exe, "16", str(mapped)], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    rows = np.array([[float(v) for v in line.split()] for line in lines if not line.startswith("#")])
    maps = [[int(v) for v in line.split()[2:]] for line in lines if line.startswith("# maps")]
    logged = [float(v) for v in [line for line in lines if line.startswith("# logged")][0].split()[2:]]
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    for f in range(mapped):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
    assert maps[0] == [s.map(L.EDGE).size, s.map(L.PLANE).size]
    assert logged == [mapped, s.logged_keypoints(0, L.PLANE).size, s.get_param("LoggedKeypointsBytes")]
    P, t, _ = s.trajectory()
    P2 = bend(P)
    s.set_trajectory(P2, t)
    assert rows.shape == (mapped + 2, 4)
    assert np.allclose(rows[:mapped, 1:4], P2[:, :3, 3], atol=1e-11, rtol=0)
    assert maps[1] == [s.map(L.EDGE).size, s.map(L.PLANE).size]
    for f in range(mapped, mapped + 2):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
        assert int(rows[f, 0]) == f
        assert np.allclose(rows[f, 1:4], s.world_transform()[:3, 3], atol=1e-9, rtol=0)
    s.close()
