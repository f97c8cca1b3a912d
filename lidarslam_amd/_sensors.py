"""Wheel odometer and gravity terms of the localization problem, and the sensor managers without a device."""
import ctypes as C

import numpy as np

from ._abi import LsaError, lib
from ._native import ptr


class SensorTerms(C.Structure):
    """lsa_sensor_terms_t (include/lidarslam_amd.h): the wheel odometer and gravity terms of the localization problem.
    ``SensorTerms(wheel_weight=1.0, d=3.0)`` turns the odometer term on, ``gravity_weight=...`` the gravity term."""

    _fields_ = [
        ("wheel", C.c_int), ("wheel_weight", C.c_double), ("p", C.c_double * 3), ("d", C.c_double),
        ("gravity", C.c_int), ("gravity_weight", C.c_double), ("g_ref", C.c_double * 3), ("g_cur", C.c_double * 3),
    ]

    def __init__(self, wheel_weight=None, p=(0.0, 0.0, 0.0), d=0.0, gravity_weight=None, g_ref=(0.0, 0.0, 1.0), g_cur=(0.0, 0.0, 1.0)):
        super().__init__()
        if wheel_weight is not None:
            self.wheel, self.wheel_weight, self.d = 1, float(wheel_weight), float(d)
            self.p[:] = [float(v) for v in p]
        if gravity_weight is not None:
            self.gravity, self.gravity_weight = 1, float(gravity_weight)
            self.g_ref[:] = [float(v) for v in g_ref]
            self.g_cur[:] = [float(v) for v in g_cur]

    def as_tuple(self):
        """every field, in order (the flags as ints): equal tuples are equal terms, bit for bit"""
        return (self.wheel, self.wheel_weight, *self.p, self.d, self.gravity, self.gravity_weight, *self.g_ref, *self.g_cur)


def sensor_terms_eval(terms, w):
    """lsa_sensor_terms_eval: the terms' 29 sums (cost, g[6], H upper triangle, count) at w, on the host (libm)"""
    w = np.ascontiguousarray(w, np.float64)
    out = np.zeros(29)
    if lib().lsa_sensor_terms_eval(C.byref(terms), ptr(w), ptr(out)) != 0:
        raise LsaError("lsa_sensor_terms_eval")
    return out


def sums_to_normal_equations(sums):
    """29 sums -> (cost, g[6], H 6x6, count)"""
    g = np.array(sums[1:7])
    H = np.zeros((6, 6))
    h = 7
    for a in range(6):
        for b in range(a, 6):
            H[a, b] = H[b, a] = sums[h]
            h += 1
    return float(sums[0]), g, H, int(sums[28])


class Sensors:
    """The wheel odometer / IMU managers of LidarSlam::Slam without a device (lsa_sensors_*)."""

    def __init__(self):
        self.L = lib()
        self.h = self.L.lsa_sensors_create()

    def close(self):
        if getattr(self, "h", None):
            self.L.lsa_sensors_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def add_wheel_odom(self, time, distance):
        self.L.lsa_sensors_add_wheel_odom(self.h, float(time), float(distance))

    def add_gravity(self, time, acc):
        a = np.ascontiguousarray(acc, np.float64)
        self.L.lsa_sensors_add_gravity(self.h, float(time), ptr(a))

    def set_weights(self, wheel, gravity):
        self.L.lsa_sensors_set_weights(self.h, float(wheel), float(gravity))

    def set_time_offset(self, offset):
        self.L.lsa_sensors_set_time_offset(self.h, float(offset))

    def clear(self):
        self.L.lsa_sensors_clear(self.h)

    def compute(self, lidar_time):
        t = SensorTerms()
        self.L.lsa_sensors_compute(self.h, float(lidar_time), C.byref(t))
        return t

    def gravity_ref(self):
        g = np.zeros(3)
        have = self.L.lsa_sensors_gravity_ref(self.h, ptr(g))
        return g, bool(have)
