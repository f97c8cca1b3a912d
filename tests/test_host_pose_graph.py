"""The host statement of the pose-graph solve (lidarslam_amd/csrc/host/lsa_pose_graph.cpp over lsa_pose_graph.h) in a stand-alone
program with its own main, built for the CPU with Address + UB sanitizer, over the shapes of the tests, the seams and the
refusals.  Nothing loaded into Python runs under a sanitizer."""
import os
import platform
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_host_statement_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "drv")
    host = os.path.join(ROOT, "lidarslam_amd", "csrc", "host")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags + ["-I" + host, os.path.join(ROOT, "tests", "pose_graph_sanitize.cpp"),
                                                                             os.path.join(host, "lsa_pose_graph.cpp"), "-o", exe]
    # whether this compiler has the sanitizers' runtime at all is decided on a program of one line; the build proper is then
    # asserted: an error in the driver or in the code under test is a failure, never a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this compiler has no runtime for -fsanitize=address,undefined")
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    # the sanitizers' fixed shadow layout does not hold an executable placed by high-entropy ASLR: the driver runs with its
    # own address space unrandomized
    norand = ["setarch", platform.machine(), "-R"]
    if shutil.which("setarch") is None or subprocess.run(norand + ["true"], capture_output=True).returncode != 0:
        norand = []
    run = subprocess.run(norand + [exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.startswith("ok"), (run.stdout[-1500:], run.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
