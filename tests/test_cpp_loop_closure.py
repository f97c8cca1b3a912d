"""examples/slam_loop_closure.cpp -- map with the keypoint log on, find a candidate, register the query frame against the log
around it, spread the correction, SetTrajectoryAndRebuildMaps, two more frames -- through the C++ mirror gives what the same
calls give through the Python front end (one C ABI).  Without a GPU the example compiles, links and refuses to run."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_loop_closure")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


def share_of(C, s):
    """the example's Share(): the translation times s, the rotation about the same axis by s times its angle"""
    w = np.array([(C[2, 1] - C[1, 2]) / 2, (C[0, 2] - C[2, 0]) / 2, (C[1, 0] - C[0, 1]) / 2])
    sine, cosine = np.sqrt(w @ w), (np.trace(C[:3, :3]) - 1) / 2
    out = np.eye(4)
    out[:3, 3] = s * C[:3, 3]
    if sine < 1e-15:
        return out
    u, a = w / sine, s * np.arctan2(sine, cosine)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    out[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    return out


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_loop_closure")
    mapped = 12
    r = subprocess.run([exe, "16", str(mapped)], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    rows = np.array([[float(v) for v in line.split()] for line in lines if not line.startswith("#")])
    extra = {line.split()[1]: [float(v) for v in line.split()[2:]] for line in lines if line.startswith("#")}
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1)
    for f in range(mapped):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
    P, t, _ = s.trajectory()
    query = mapped - 3
    revisited = L.loop_closure_candidate(P, t, query, 2.2, 4.0)
    assert extra["candidate"] == [query, revisited] and 0 <= revisited < query - 2
    reg = s.register_logged_frames(query, revisited, L.LoopClosureParams(revisited_half_window=2))
    assert extra["registered"] == [reg.status, reg.iterations, reg.target_points[L.EDGE], reg.target_points[L.PLANE], reg.query_points[L.EDGE], reg.query_points[L.PLANE]]
    assert reg.status == 0 and reg.target_points[L.PLANE] > 1000
    assert np.allclose(extra["world"], reg.world[:3, 3], atol=1e-9, rtol=0)
    assert np.allclose(extra["relative"], reg.relative[:3, 3], atol=1e-9, rtol=0)
    assert np.allclose(extra["errors"], [reg.position_error, reg.orientation_error], atol=1e-8, rtol=0)
    C = reg.world @ np.linalg.inv(P[query])
    P2 = P.copy()
    for i in range(revisited + 1, mapped):
        P2[i] = share_of(C, 1.0 if i >= query else (i - revisited) / (query - revisited)) @ P[i]
    s.set_trajectory(P2, t)
    assert rows.shape == (mapped + 2, 4)
    assert np.allclose(rows[:mapped, 1:4], P2[:, :3, 3], atol=1e-9, rtol=0)
    assert np.abs(P2[query] - reg.world).max() < 1e-9  # the query pose is where the registration put it
    for f in range(mapped, mapped + 2):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
        assert int(rows[f, 0]) == f
        assert np.allclose(rows[f, 1:4], s.world_transform()[:3, 3], atol=1e-7, rtol=0)
    s.close()
