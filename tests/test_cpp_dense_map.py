"""examples/slam_dense_map.cpp -- a short drive mapped with SetDenseMap(1), saved with minFrames 1 and 3 -- through the C++
mirror writes the files the Python front end's map of the same drive gives (both sit on the same C ABI)."""
import subprocess

import pytest

from test_cpp_api import build_example


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map")
    frames, leaf = 6, 0.2
    r = subprocess.run([exe, str(tmp_path), "16", str(frames), str(leaf), "1"], capture_output=True, text=True, check=True)
    extra = {line.split()[1]: [int(v) for v in line.split()[2:]] for line in r.stdout.strip().splitlines() if line.startswith("#")}
    s = L.Slam(0, EgoMotion=3, DenseMapLeafSize=leaf, DenseMap=1)
    for f in range(frames):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
    everything, three = L.dense_map(s, 1)[0], L.dense_map(s, 3)[0]
    assert extra["dense"] == extra["fetched"] == [everything.size, three.size] and 100 < three.size < everything.size
    assert L.read_pcd(str(tmp_path / "dense.pcd")).tobytes() == everything.tobytes()
    assert L.read_pcd(str(tmp_path / "dense_3.pcd")).tobytes() == three.tobytes()
    for m, name in ((1, "dense.pcd"), (3, "dense_3.pcd")):
        assert L.save_dense_map_pcd(s, str(tmp_path / ("py_" + name)), 1, m) > 0
        assert open(str(tmp_path / ("py_" + name)), "rb").read() == open(str(tmp_path / name), "rb").read()
    s.close()
