"""examples/slam_dense_map_grid.cpp -- a short drive mapped with SetDenseMap(1) and SetDenseMapCarve(1), rasterised into the
whole plan and the local costmap around the last pose, both saved for map_server -- through the C++ mirror gives what the
Python front end gives for the same drive (both sit on the same C ABI)."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_grid")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_grid")
    frames, leaf, half = 6, 0.2, 10.0
    r = subprocess.run([exe, str(tmp_path), "16", str(frames), str(leaf), str(half)], capture_output=True, text=True, check=True)
    extra = {line.split()[1]: [int(v) for v in line.split()[2:]] for line in r.stdout.strip().splitlines() if line.startswith("#")}
    s = L.Slam(0, EgoMotion=3, DenseMapLeafSize=leaf, DenseMap=1, DenseMapCarve=1)
    for f in range(frames):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
    for name, grid in (("plan", L.dense_map_grid(s, max_miss_ratio=1.0)), ("local", L.dense_map_grid(s, max_miss_ratio=1.0, half_extent=half))):
        info, _, state = grid
        counts = [int((state == v).sum()) for v in (100, 0, -1)]
        assert extra[name] == [int(info["width"]), int(info["height"])] + counts and min(counts) > 0, name
        back, resolution, origin = L.read_occupancy_pgm(str(tmp_path / name))
        assert back.tobytes() == state.tobytes() and resolution == float(info["resolution"]) == 2 * leaf
        assert origin == (float(info["origin_x"]), float(info["origin_y"]))
    assert np.prod(extra["local"][:2]) < np.prod(extra["plan"][:2])
    s.close()
