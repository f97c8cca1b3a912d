"""examples/slam_dense_map_changes.cpp -- a short drive mapped with SetDenseMap(1), a box of points no earlier frame holds added
to the next frame, CompareFrameToDenseMap and RenderDenseMapScan through the C++ mirror: the box's points are UNMAPPED, the
counts are the Python front end's for the same frames (both sit on the same C ABI), and the rendered scan hits the map."""
import subprocess

import numpy as np
import pytest

from test_cpp_api import build_example


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_changes")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_labels_the_box_unmapped_and_matches_the_python_front_end(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_changes")
    frames, leaf, box = 6, 0.2, 40
    r = subprocess.run([exe, "16", str(frames), str(leaf), str(box)], capture_output=True, text=True, check=True)
    out = {line.split()[1]: [int(v) for v in line.split()[2:]] for line in r.stdout.strip().splitlines() if line.startswith("#")}
    assert out["box"] == [box, box]  # every point of the box is UNMAPPED
    assert out["scan"][0] == 16 * 360 and out["scan"][1] > 1000
    # the same frames through the Python front end
    s = L.Slam(0, EgoMotion=3, DenseMapLeafSize=leaf, DenseMap=1)
    for f in range(frames + 1):
        pts, stamp = L.synth_frame(16, 1000, f)
        if f == frames:
            own = pts.size
            extra = np.repeat(pts[own // 2: own // 2 + 1], box)
            i = np.arange(box)
            extra["x"] = np.float32(5.5) + (i % 5).astype(np.float32) * np.float32(0.25)
            extra["y"] = np.float32(-0.5) + ((i // 5) % 4).astype(np.float32) * np.float32(0.33)
            extra["z"] = np.float32(-0.5) + (i // 20).astype(np.float32) * np.float32(0.9)
            extra["laser_id"] = i % 16
            pts = np.concatenate([pts, extra])
        s.add_frame(pts, stamp, f)
    labels, counts = L.dense_map_compare_frame(s)
    assert counts.tolist() == out["labels"] and (labels[own:] == 2).all()
    assert counts[1] > (counts.sum() - counts[0]) // 2  # more than half the judged points are CONSISTENT
    el = np.deg2rad(-15.0 + 2.0 * np.arange(16))
    assert int((L.dense_map_render_scan(s, el, 360)["status"] == 1).sum()) == out["scan"][1]
    s.close()
