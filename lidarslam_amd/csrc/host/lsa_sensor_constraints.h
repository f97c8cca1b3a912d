// lsa_sensor_constraints.h -- the external sensor managers of LidarSlam::Slam (slam_lib/include/LidarSlam/SensorConstraints.h,
// slam_lib/src/SensorConstraints.cxx): a wheel odometer (absolute mode, ComputeWheelAbsoluteConstraint) and an IMU
// (ComputeGravityConstraint, ComputeGravityRef).  They turn the measurements held at a frame's LiDAR time into the
// lsa_sensor_terms_t the localization solve adds to its normal equations (lsa_sensor_terms.h).
//
// Defined where the reference reads out of bounds:
//   * the LiDAR time equals the first measurement's time (the reference's index -1): measurement 0 is used;
//   * a single measurement: its value is used;
//   * two measurements with the same time around the LiDAR time (the reference divides 0 by 0): the earlier one is used;
//   * phi = pi / theta = pi in the gravity histogram (index NPhi / NTheta): the last bin; z outside [-1, 1] after the
//     normalisation (acos NaN): clamped first.
// Norms are sqrt((x x + y y) + z z), normalisation divides every component by the norm, and only when it is > 0.
#pragma once
#include <vector>
#include "../../../include/lidarslam_amd.h"

namespace lsa
{
namespace host
{

class SensorConstraints
{
public:
  SensorConstraints() { Clear(); }
  void AddWheelOdom(double time, double distance) { Wheel.push_back({time, distance}); }
  void AddGravity(double time, const double acc[3]) { Imu.push_back({time, {acc[0], acc[1], acc[2]}}); }
  void SetWheelOdomWeight(double w) { WheelWeight = w; }
  double GetWheelOdomWeight() const { return WheelWeight; }
  void SetGravityWeight(double w) { GravityWeight = w; }
  double GetGravityWeight() const { return GravityWeight; }
  // Slam::SetSensorTimeOffset sets the offset of both managers, the getter returns the IMU's (they never differ)
  void SetTimeOffset(double t) { TimeOffset = t; }
  double GetTimeOffset() const { return TimeOffset; }
  // Slam::ClearSensorMeasurements -> SensorManager::Reset of both: measurements and residuals cleared, PreviousIdx -1,
  // time offset 0; the gravity reference and the odometer's PreviousDistance are kept
  void Clear();
  // SensorManager::CanBeUsed of either manager
  bool CanBeUsed() const { return WheelUsable() || ImuUsable(); }
  // Slam::AddFrames (Slam.cxx:256-261, 347-352): when either manager is usable, both compute their residual at the
  // frame's LiDAR time; otherwise nothing is computed and the previous frame's terms (with their weights) stay
  const lsa_sensor_terms_t& Compute(double lidarTime);
  const lsa_sensor_terms_t& Terms() const { return Current; }
  // the gravity reference: zero until the IMU needed it the first time
  const double* GravityRef() const { return GRef; }

private:
  struct WheelMeasure { double Time, Distance; };
  struct ImuMeasure { double Time; double Acc[3]; };
  std::vector<WheelMeasure> Wheel;
  std::vector<ImuMeasure> Imu;
  double WheelWeight = 0., GravityWeight = 0., TimeOffset = 0.;
  int WheelPrevIdx = -1, ImuPrevIdx = -1;
  double PreviousDistance = 0.;
  double GRef[3] = {0., 0., 0.};
  lsa_sensor_terms_t Current;
  bool WheelUsable() const { return WheelWeight > 1e-6 && !Wheel.empty(); }
  bool ImuUsable() const { return GravityWeight > 1e-6 && !Imu.empty(); }
  void ComputeWheel(double lidarTime);
  void ComputeGravity(double lidarTime);
  void ComputeGravityRef(double deltaAngle);
};

}  // namespace host
}  // namespace lsa
