// The sequence of sensor calls the ParaView wrapper makes on LidarSlam::Slam (vtkSlam.cxx:211-213, 406-453): the
// measurements read from a file are handed over after ClearSensorMeasurements, the time offset is set on every frame,
// the weights come from the proxies.  Wheel odometer (arc length of the synthetic path, +3 %) and IMU (gravity along +z)
// at 100 Hz.
//   ./slam_sensor_calls [model=16] [frames=12]      prints "frame x y z roll" of every pose
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "LidarSlam/Slam.h"

namespace
{
// arc length of the synthetic path (lsa_synth.cpp: 5 m/s, 3 degrees of yaw at 0.1 Hz), Simpson's rule
double ArcLength(double t)
{
  const double speed = 5.0, amp = 3.0 * M_PI / 180.0, omega = 2.0 * M_PI / 10.0;
  const int n = 2 * std::max(1, (int)std::ceil(t / 1e-3));
  const double h = t / n;
  double s = 0.;
  for (int i = 0; i <= n; ++i)
  {
    const double v = std::sqrt(speed * speed + std::pow(speed * amp * std::sin(omega * i * h), 2));
    s += (i == 0 || i == n) ? v : (i % 2 ? 4 * v : 2 * v);
  }
  return s * h / 3;
}
}  // namespace

int main(int argc, char** argv)
{
  const int model = argc > 1 ? std::atoi(argv[1]) : 16;
  const int nframes = argc > 2 ? std::atoi(argv[2]) : 12;
  try
  {
    LidarSlam::Slam slam;
    slam.SetEgoMotion(LidarSlam::EgoMotionMode::MOTION_EXTRAPOLATION_AND_REGISTRATION);
    // vtkSlam::SetSensorData: a new file replaces the measurements held
    slam.ClearSensorMeasurements();
    for (int k = 0; k < 400; ++k)
    {
      LidarSlam::SensorConstraints::WheelOdomMeasurement w;
      w.Time = 0.01 * k;
      w.Distance = 1.03 * ArcLength(w.Time);
      slam.AddWheelOdomMeasurement(w);
      LidarSlam::SensorConstraints::GravityMeasurement g;
      g.Time = 0.01 * k;
      g.Acceleration[0] = 0.;
      g.Acceleration[1] = 0.;
      g.Acceleration[2] = 9.81;
      slam.AddGravityMeasurement(g);
    }
    slam.SetWheelOdomWeight(50.);
    slam.SetGravityWeight(100.);
    for (int f = 0; f < nframes; ++f)
    {
      LidarSlam::Slam::PointCloud::Ptr pc(new LidarSlam::Slam::PointCloud);
      pc->points.resize(1 << 19);
      std::uint64_t stamp = 0;
      const int n = lsa_synth_frame(model, 1000, f, reinterpret_cast<lsa_point_t*>(pc->points.data()), (int)pc->points.size(), &stamp);
      if (n < 0) return 2;
      pc->points.resize(n);
      pc->header.stamp = stamp;
      pc->header.seq = f;
      slam.SetSensorTimeOffset(0.);  // vtkSlam::RequestData, every frame
      slam.AddFrame(pc);
      const LidarSlam::Transform T = slam.GetWorldTransform();
      const auto& M = T.GetMatrixArray();
      std::printf("%d %.12f %.12f %.12f %.12f\n", f, T.x(), T.y(), T.z(), std::atan2(M[9], M[10]));
    }
    std::printf("# weights %g %g %g\n", slam.GetWheelOdomWeight(), slam.GetGravityWeight(), slam.GetSensorTimeOffset());
  }
  catch (const std::exception& e)
  {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
