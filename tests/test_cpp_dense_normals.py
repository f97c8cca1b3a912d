"""examples/slam_dense_map_normals.cpp -- a short drive mapped with SetDenseMap(1) and SetDenseMapCarve(1), saved with normals,
filtered at ratio 1, radius 2, oriented -- through the C++ mirror writes the file the Python front end gives for the same drive
(both sit on the same C ABI)."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_normals")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_normals")
    frames, leaf = 6, 0.2
    r = subprocess.run([exe, str(tmp_path), "16", str(frames), str(leaf), "1"], capture_output=True, text=True, check=True)
    extra = {line.split()[1]: [int(v) for v in line.split()[2:]] for line in r.stdout.strip().splitlines() if line.startswith("#")}
    s = L.Slam(0, EgoMotion=3, DenseMapLeafSize=leaf, DenseMap=1, DenseMapCarve=1)
    for f in range(frames):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
    path = str(tmp_path / "python.pcd")
    seen, normals = L.dense_map_filtered(s, 1, 1.0)[0], L.dense_map_normals(s, 1, 1.0, 2, 5, True)
    assert L.save_dense_map_pcd_normals(s, path, 1, 1, 1.0, 2, 5, True) == seen.size == len(normals) > 100
    theirs = str(tmp_path / "dense_normals.pcd")
    assert open(theirs, "rb").read() == open(path, "rb").read()
    assert L.read_pcd(theirs).tobytes() == seen.tobytes()
    four = L.read_pcd_normals(theirs)
    assert four.view(np.uint32).tobytes() == np.stack([normals[a].view(np.uint32) for a in ("normal_x", "normal_y", "normal_z", "curvature")], axis=1).tobytes()
    without = int(np.isnan(normals["normal_x"]).sum())
    assert extra["normals"] == [seen.size, without] and without < seen.size
    s.close()
