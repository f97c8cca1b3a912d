// lsa_sensor_constraints.cpp -- the wheel odometer and IMU managers (SensorConstraints.cxx restated, see the header for
// the cases defined where the reference reads out of bounds) and their GPU-free C ABI: lsa_sensors_* for the tests,
// lsa_sensor_terms_eval (the shared residual arithmetic of lsa_sensor_terms.h with libm's sin / cos).
#include "lsa_sensor_constraints.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include "../lsa_accum.h"
#include "../lsa_sensor_terms.h"

namespace lsa
{
namespace host
{

namespace
{
double Norm3(const double v[3]) { return std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
// Eigen's normalized(): v / |v|, unchanged when |v| is 0
void Normalized(const double v[3], double o[3])
{
  const double sq = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  if (sq > 0.)
  {
    const double n = std::sqrt(sq);
    for (int i = 0; i < 3; ++i) o[i] = v[i] / n;
  }
  else
    for (int i = 0; i < 3; ++i) o[i] = v[i];
}
// the last measurement at or before t (t within [front, back]), from the one the previous frame used:
// while (Measures[idx + 1].Time < t) ++idx, then idx -1 (t is the first time) -> 0
template <typename M>
int IndexBefore(const std::vector<M>& m, int prev, double t)
{
  int idx = prev;
  while (idx + 1 < (int)m.size() && m[idx + 1].Time < t) ++idx;
  return std::max(idx, 0);
}
// interpolation ratio between measurements idx and idx + 1 (0: no second one, or both at the same time)
template <typename M>
double Ratio(const std::vector<M>& m, int idx, double t)
{
  if (idx + 1 >= (int)m.size()) return 0.;
  const double dt = m[idx + 1].Time - m[idx].Time;
  return dt > 0. ? (t - m[idx].Time) / dt : 0.;
}
}  // namespace

void SensorConstraints::Clear()
{
  Wheel.clear();
  Imu.clear();
  WheelPrevIdx = -1;
  ImuPrevIdx = -1;
  TimeOffset = 0.;
  std::memset(&Current, 0, sizeof(Current));
}

const lsa_sensor_terms_t& SensorConstraints::Compute(double lidarTime)
{
  if (!CanBeUsed()) return Current;  // quirk: the previous frame's residuals stay in the problem
  ComputeWheel(lidarTime);
  ComputeGravity(lidarTime);
  return Current;
}

// WheelOdometryManager::ComputeWheelAbsoluteConstraint (SensorConstraints.cxx:8-54)
void SensorConstraints::ComputeWheel(double lidarTime)
{
  Current.wheel = 0;
  Current.wheel_weight = 0.;
  Current.p[0] = Current.p[1] = Current.p[2] = 0.;
  Current.d = 0.;
  if (!WheelUsable()) return;
  lidarTime -= TimeOffset;
  if (lidarTime < Wheel.front().Time || lidarTime > Wheel.back().Time) return;  // no measurement around the frame
  if (WheelPrevIdx >= 0 && Wheel[WheelPrevIdx].Time > lidarTime) WheelPrevIdx = -1;  // the timeline went back
  const int idx = IndexBefore(Wheel, WheelPrevIdx, lidarTime);
  const double rt = Ratio(Wheel, idx, lidarTime);
  const double next = idx + 1 < (int)Wheel.size() ? Wheel[idx + 1].Distance : Wheel[idx].Distance;
  const double distance = (1 - rt) * Wheel[idx].Distance + rt * next;
  if (WheelPrevIdx == -1)
  {
    // the first frame with a measurement: no constraint, the distance is the baseline from now on
    WheelPrevIdx = idx;
    PreviousDistance = distance;
    return;
  }
  // OdometerDistanceResidual from PreviousPose -- never set by Slam: the identity, p = 0
  Current.wheel = 1;
  Current.wheel_weight = WheelWeight;
  Current.d = distance - PreviousDistance;
  WheelPrevIdx = idx;
}

// ImuManager::ComputeGravityConstraint (SensorConstraints.cxx:104-145)
void SensorConstraints::ComputeGravity(double lidarTime)
{
  Current.gravity = 0;
  Current.gravity_weight = 0.;
  for (int i = 0; i < 3; ++i) Current.g_ref[i] = Current.g_cur[i] = 0.;
  if (!ImuUsable()) return;
  lidarTime -= TimeOffset;
  if (lidarTime < Imu.front().Time || lidarTime > Imu.back().Time) return;
  // Utils::Deg2Rad(5.f): 5 / 180 * pi worked out in double, returned as float
  if (Norm3(GRef) < 1e-6) ComputeGravityRef(static_cast<double>(static_cast<float>(5.0 / 180. * M_PI)));
  if (ImuPrevIdx >= 0 && Imu[ImuPrevIdx].Time > lidarTime) ImuPrevIdx = -1;
  const int idx = IndexBefore(Imu, ImuPrevIdx, lidarTime);
  const double rt = Ratio(Imu, idx, lidarTime);
  double a[3], b[3], g[3];
  Normalized(Imu[idx].Acc, a);
  Normalized(Imu[idx + 1 < (int)Imu.size() ? idx + 1 : idx].Acc, b);
  for (int i = 0; i < 3; ++i) g[i] = (1 - rt) * a[i] + rt * b[i];
  const double n = Norm3(g);
  if (!(n > 1e-6)) return;  // an inconsistent IMU measurement
  Current.gravity = 1;
  Current.gravity_weight = GravityWeight;
  for (int i = 0; i < 3; ++i)
  {
    Current.g_ref[i] = GRef[i];
    Current.g_cur[i] = g[i] / n;
  }
  ImuPrevIdx = idx;
}

// ImuManager::ComputeGravityRef (SensorConstraints.cxx:147-186): the mean direction of the fullest (phi, theta) bin of a
// histogram over every measurement held (the first fullest bin in (phi, theta) order)
void SensorConstraints::ComputeGravityRef(double deltaAngle)
{
  const int nPhi = static_cast<int>(std::ceil(2 * M_PI / deltaAngle));
  const int nTheta = static_cast<int>(std::ceil(M_PI / deltaAngle));
  std::vector<int> count((size_t)nPhi * nTheta, 0), bin(Imu.size());
  for (size_t i = 0; i < Imu.size(); ++i)
  {
    double d[3];
    Normalized(Imu[i].Acc, d);
    const int ip = std::min(static_cast<int>((std::atan2(d[1], d[0]) + M_PI) / deltaAngle), nPhi - 1);
    const int it = std::min(static_cast<int>(std::acos(std::min(std::max(d[2], -1.), 1.)) / deltaAngle), nTheta - 1);
    bin[i] = ip * nTheta + it;
    ++count[bin[i]];
  }
  int best = 0;
  for (int k = 0; k < nPhi * nTheta; ++k)
    if (count[k] > count[best]) best = k;
  double s[3] = {0., 0., 0.};
  for (size_t i = 0; i < Imu.size(); ++i)
    if (bin[i] == best)
    {
      double d[3];
      Normalized(Imu[i].Acc, d);
      for (int j = 0; j < 3; ++j) s[j] += d[j];
    }
  Normalized(s, GRef);
}

}  // namespace host
}  // namespace lsa

using lsa::host::SensorConstraints;

struct lsa_sensors
{
  SensorConstraints m;
};

extern "C" {

int lsa_sensor_terms_eval(const lsa_sensor_terms_t* terms, const double w[6], double sums[29])
{
  if (!terms || !w || !sums) return LSA_E_ARG;
  double R[9], dRx[9], dRy[9], dRz[9];
  lsa::rotation_and_derivatives(std::cos(w[3]), std::sin(w[3]), std::cos(w[4]), std::sin(w[4]), std::cos(w[5]), std::sin(w[5]), R, dRx, dRy, dRz);
  for (int v = 0; v < 29; ++v) sums[v] = 0.;
  lsa::sensor_terms_add(*terms, w, R, dRx, dRy, dRz, true, sums);
  return LSA_OK;
}

lsa_sensors* lsa_sensors_create(void) { return new lsa_sensors(); }
void lsa_sensors_destroy(lsa_sensors* s) { delete s; }

int lsa_sensors_add_wheel_odom(lsa_sensors* s, double time, double distance)
{
  if (!s) return LSA_E_ARG;
  s->m.AddWheelOdom(time, distance);
  return LSA_OK;
}

int lsa_sensors_add_gravity(lsa_sensors* s, double time, const double acc[3])
{
  if (!s || !acc) return LSA_E_ARG;
  s->m.AddGravity(time, acc);
  return LSA_OK;
}

int lsa_sensors_set_weights(lsa_sensors* s, double wheel_weight, double gravity_weight)
{
  if (!s) return LSA_E_ARG;
  s->m.SetWheelOdomWeight(wheel_weight);
  s->m.SetGravityWeight(gravity_weight);
  return LSA_OK;
}

int lsa_sensors_set_time_offset(lsa_sensors* s, double offset)
{
  if (!s) return LSA_E_ARG;
  s->m.SetTimeOffset(offset);
  return LSA_OK;
}

int lsa_sensors_clear(lsa_sensors* s)
{
  if (!s) return LSA_E_ARG;
  s->m.Clear();
  return LSA_OK;
}

int lsa_sensors_compute(lsa_sensors* s, double lidar_time, lsa_sensor_terms_t* out)
{
  if (!s || !out) return LSA_E_ARG;
  *out = s->m.Compute(lidar_time);
  return LSA_OK;
}

int lsa_sensors_gravity_ref(const lsa_sensors* s, double g[3])
{
  if (!s || !g) return LSA_E_ARG;
  const double* r = s->m.GravityRef();
  for (int i = 0; i < 3; ++i) g[i] = r[i];
  return (r[0] != 0. || r[1] != 0. || r[2] != 0.) ? 1 : 0;
}

}  // extern "C"
