"""examples/slam_dense_map_loops.cpp -- the forward-and-back drive mapped with SetDenseMap(1) and SetDenseMapOnTrajectory(1), its
loops closed with CloseLoops and apply, the dense map saved before and after -- compiles and links against the C++ mirror;
without a GPU it refuses to run; on one it writes the files the Python front end's map of the same drive gives."""
import subprocess

import pytest

from test_cpp_api import build_example

MODEL, FORWARD, LEAF = 16, 12, 0.2


def test_the_example_compiles_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_loops")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr


@pytest.mark.gpu
def test_the_example_keeps_the_map_the_python_front_end_keeps(tmp_path, L):
    exe = build_example(tmp_path, "slam_dense_map_loops")
    r = subprocess.run([exe, str(tmp_path), str(MODEL), str(FORWARD), str(LEAF)], capture_output=True, text=True, check=True)
    extra = {line.split()[1]: [int(v) for v in line.split()[2:]] for line in r.stdout.strip().splitlines() if line.startswith("#")}
    frames = [L.synth_frame(MODEL, 1000, f) for f in range(FORWARD)]
    order = list(range(FORWARD)) + list(range(FORWARD - 2, -1, -1))
    period = frames[1][1] - frames[0][1]
    s = L.Slam(0, EgoMotion=3, LoggingTimeout=-1, DenseMapLeafSize=LEAF, DenseMap=1, DenseMapOnTrajectory=1)
    for f, c in enumerate(order):
        s.add_frame(frames[c][0], frames[0][1] + f * period, f)
    before = L.dense_map(s)[0]
    rb = L.PoseGraphRobust(edge_loss=L.PGO_LOSS_TUKEY, edge_scale=3.0)
    _, _, _, reports = L.close_loops(s, rb, L.LoopClosureParams(revisited_half_window=2), apply=True, min_travelled=2.0, max_distance=0.0, exclusion_half_window=2,
                                     first_query=FORWARD + 2, query_stride=3)
    after, sources = L.dense_map(s)[0], L.dense_map_sources(s)
    assert extra["before"] == [before.size] and before.size > 5000
    assert extra["loops"] == [len(reports), sum(r.edge >= 0 for r in reports)] and extra["loops"][1] >= 1
    assert extra["after"] == [after.size, int(s.get_param("DenseMapDropped")), 1, 0] and 0 < after.size <= before.size
    assert extra["sources"] == [sources.size, int(sources.min()), int(sources.max())] and sources.size == after.size and sources.max() < len(order)
    assert L.read_pcd(str(tmp_path / "dense_before.pcd")).tobytes() == before.tobytes()
    assert L.read_pcd(str(tmp_path / "dense.pcd")).tobytes() == after.tobytes()
    assert before.tobytes() != after.tobytes()  # the loops moved the poses, and the map with them
    s.close()
