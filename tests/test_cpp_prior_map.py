"""examples/slam_prior_map.cpp -- map, save, load into a fresh LidarSlam::Slam with MapUpdate = NONE, localize -- through the
C++ mirror gives the poses of the same calls through the Python front end (both sit on the same C ABI)."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_prior_map")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe, str(tmp_path / "m_")], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [1, 2])
def test_the_example_matches_the_python_front_end(tmp_path, L, fmt):
    exe = build_example(tmp_path, "slam_prior_map")
    mapped, localized = 6, 3
    r = subprocess.run([exe, str(tmp_path / "cpp_"), "16", str(mapped), str(localized), str(fmt)], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    rows = np.array([[float(v) for v in line.split()] for line in lines if not line.startswith("#")])
    extra = {line.split()[1]: [int(v) for v in line.split()[2:]] for line in lines if line.startswith("#")}
    assert "LidarSlam::Slam::SaveMapsToPCD" in r.stderr and "LidarSlam::Slam::LoadMapsFromPCD" in r.stderr and "cpp_planes.pcd (" in r.stderr
    a = L.Slam(0, EgoMotion=3, VoxelGridMinFramesPerVoxel=1)
    for f in range(mapped):
        pts, stamp = L.synth_frame(16, 1000, f)
        a.add_frame(pts, stamp, f)
    where = a.world_transform()
    prefix = str(tmp_path / "py_")
    counts = a.save_maps_pcd(prefix, fmt, filtered=False)
    a.close()
    b = L.Slam(0, EgoMotion=3, VoxelGridMinFramesPerVoxel=1, MapUpdate=0)
    assert b.load_maps_pcd(prefix) == counts
    b.set_world_transform_from_guess(where)
    assert rows.shape == (localized, 4)
    for i, f in enumerate(range(mapped, mapped + localized)):
        pts, stamp = L.synth_frame(16, 1000, f)
        b.add_frame(pts, stamp, f)
        assert int(rows[i, 0]) == f
        assert np.allclose(rows[i, 1:4], b.world_transform()[:3, 3], atol=1e-11, rtol=0)
    assert extra["maps"] == [b.map(L.EDGE).size, b.map(L.PLANE).size] == counts[:2]
    # the two front ends wrote the same files
    for name in ("edges.pcd", "planes.pcd"):
        assert open(str(tmp_path / ("cpp_" + name)), "rb").read() == open(prefix + name, "rb").read()
    b.close()
