"""The C++ mirror's sensor calls (examples/slam_sensor_calls.cpp, the ParaView wrapper's sequence) reach the library:
the poses equal those of the Python front-end making the same calls."""
import math

import numpy as np
import pytest

from test_cpp_api import build_example


def arc_length(t):
    speed, amp, omega = 5.0, 3.0 * math.pi / 180.0, 2.0 * math.pi / 10.0
    n = 2 * max(1, math.ceil(t / 1e-3))
    h = t / n
    s = 0.0
    for i in range(n + 1):
        v = math.sqrt(speed * speed + math.pow(speed * amp * math.sin(omega * i * h), 2))
        s += v if i in (0, n) else (4 * v if i % 2 else 2 * v)
    return s * h / 3


def test_sensor_calls_compile_against_the_mirror(tmp_path, L):
    build_example(tmp_path, "slam_sensor_calls")


@pytest.mark.gpu
def test_sensor_calls_match_the_python_front_end(tmp_path, L):
    import subprocess

    exe = build_example(tmp_path, "slam_sensor_calls")
    r = subprocess.run([exe, "16", "12"], capture_output=True, text=True, check=True)
    lines = r.stdout.strip().splitlines()
    rows = np.array([[float(v) for v in line.split()] for line in lines if not line.startswith("#")])
    assert [line for line in lines if line.startswith("# weights")] == ["# weights 50 100 0"]
    # the measurements came before the weights (the wrapper's order): one warning per method
    assert r.stderr.count("AddWheelOdomMeasurement: stored; no constraint while the weight is 0") == 1
    assert r.stderr.count("AddGravityMeasurement: stored; no constraint while the weight is 0") == 1
    s = L.Slam(0, EgoMotion=3)
    s.clear_sensor_measurements()
    for k in range(400):
        s.add_wheel_odom(0.01 * k, 1.03 * arc_length(0.01 * k))
        s.add_gravity(0.01 * k, [0.0, 0.0, 9.81])
    s.set_param("WheelOdomWeight", 50.0)
    s.set_param("GravityWeight", 100.0)
    for f in range(12):
        pts, stamp = L.synth_frame(16, 1000, f)
        s.set_param("SensorTimeOffset", 0.0)
        s.add_frame(pts, stamp, f)
        T = s.world_transform()
        assert np.allclose(rows[f, 1:4], T[:3, 3], atol=1e-11, rtol=0)
        assert abs(rows[f, 4] - math.atan2(T[2, 1], T[2, 2])) < 1e-11
    t = s.sensor_terms()
    assert t.wheel == 1 and t.gravity == 1 and t.wheel_weight == 50.0 and t.gravity_weight == 100.0
    s.close()
