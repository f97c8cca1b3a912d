"""examples/slam_dense_map_carve.cpp -- a short drive mapped with SetDenseMap(1) and SetDenseMapCarve(1), saved unfiltered,
filtered at ratio 1 and after a prune -- through the C++ mirror writes the files the Python front end gives for the same drive
(both sit on the same C ABI)."""
import subprocess

import pytest

from test_cpp_api import build_example


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_carve")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_carve")
    frames, leaf = 6, 0.2
    r = subprocess.run([exe, str(tmp_path), "16", str(frames), str(leaf), "1"], capture_output=True, text=True, check=True)
    extra = {line.split()[1]: [int(v) for v in line.split()[2:]] for line in r.stdout.strip().splitlines() if line.startswith("#")}
    s = L.Slam(0, EgoMotion=3, DenseMapLeafSize=leaf, DenseMap=1, DenseMapCarve=1)
    for f in range(frames):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.add_frame(pts, stamp, f)
    everything, seen = L.dense_map(s, 1)[0], L.dense_map_filtered(s, 1, 1.0)[0]
    assert L.read_pcd(str(tmp_path / "dense_all.pcd")).tobytes() == everything.tobytes()
    assert L.read_pcd(str(tmp_path / "dense_seen.pcd")).tobytes() == seen.tobytes()
    removed = L.prune_dense_map(s, 1, 1.0)
    left = L.dense_map(s, 1)[0]
    assert left.tobytes() == seen.tobytes() and L.read_pcd(str(tmp_path / "dense_pruned.pcd")).tobytes() == left.tobytes()
    assert extra["carve"] == [everything.size, seen.size, left.size] and 100 < seen.size < everything.size
    assert extra["pruned"] == [removed, int(s.get_param("DenseMapRays"))] and removed == everything.size - seen.size and extra["pruned"][1] > 0
    s.close()
