"""examples/slam_close_loops.cpp -- map forward and back with the keypoint log on, find every loop closure of the log and close
them in one CloseLoops call under Tukey's loss, go on -- compiles and links against the C++ mirror; without a GPU it refuses to
run.  What it prints on a GPU is held to the Python front end in tests/test_gpu_loop_detect.py."""
import subprocess

from test_cpp_api import build_example


def test_the_example_compiles_links_and_refuses_to_run_without_a_gpu(tmp_path, L):
    exe = build_example(tmp_path, "slam_close_loops")
    if L.lib().lsa_device_count() == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 1 and "no usable HIP device" in r.stderr
