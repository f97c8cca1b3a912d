// lsa_sensor_terms.h -- the external sensor residuals of the localization problem, added to the 29 sums of the normal
// equations (cost, g[6], H upper triangle row by row, count).  Shared by the one-launch solve (k_lm_solve, once per
// evaluation after the fixed-order fold), lsa_accumulate (after its reduction) and lsa_sensor_terms_eval (host, libm).
//
//   wheel    r = |t - p| - d             OdometerDistanceResidual (CeresCostFunctions.h:255-293): |t - p| is the
//                                        constant 0 where |t - p|^2 < 1e-6, so there r = -d and J = 0
//   gravity  r = R(rx, ry, rz) gc - gr   ImuGravityAlignmentResidual (CeresCostFunctions.h:295-341), rotation only
//   loss     ScaledLoss(NULL, weight):   rho0 = weight s, rho1 = weight
// with the convention of accumulate_one (lsa_accum.h): cost += 1/2 rho0, g += rho1 J^T r, H += rho1 J^T J.  The count
// (sum 28) is the LiDAR matches alone: the minimum-matches test does not see these terms.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/lidarslam_amd.h"

namespace lsa
{

// R, dR/drx, dR/dry, dR/drz at w (rotation_and_derivatives), t = w[0..2]; jac = 0: the cost alone
__host__ __device__ inline void sensor_terms_add(const lsa_sensor_terms_t& s, const double t[3], const double R[9], const double dRx[9], const double dRy[9],
                                                 const double dRz[9], bool jac, double sums[29])
{
  if (s.wheel)
  {
    const double dx = t[0] - s.p[0], dy = t[1] - s.p[1], dz = t[2] - s.p[2];
    const double sq = (dx * dx + dy * dy) + dz * dz;
    const bool live = !(sq < 1e-6);
    const double n = live ? __builtin_sqrt(sq) : 0.0;
    const double r = n - s.d;
    const double w = s.wheel_weight;
    sums[0] += 0.5 * (w * (r * r));
    if (jac && live)
    {
      const double J[3] = {dx / n, dy / n, dz / n};
      // rows 0..2 of the upper triangle: H(a, b) at 7 + a * 6 - a (a - 1) / 2 + (b - a)
      const int row[3] = {7, 13, 18};
      for (int a = 0; a < 3; ++a)
      {
        sums[1 + a] += w * (J[a] * r);
        for (int b = a; b < 3; ++b) sums[row[a] + (b - a)] += w * (J[a] * J[b]);
      }
    }
  }
  if (s.gravity)
  {
    const double* gc = s.g_cur;
    const double r0 = ((R[0] * gc[0] + R[1] * gc[1]) + R[2] * gc[2]) - s.g_ref[0];
    const double r1 = ((R[3] * gc[0] + R[4] * gc[1]) + R[5] * gc[2]) - s.g_ref[1];
    const double r2 = ((R[6] * gc[0] + R[7] * gc[1]) + R[8] * gc[2]) - s.g_ref[2];
    const double w = s.gravity_weight;
    sums[0] += 0.5 * (w * ((r0 * r0 + r1 * r1) + r2 * r2));
    if (jac)
    {
      // column 3 + k of J = dR/drk gc
      const double* dR[3] = {dRx, dRy, dRz};
      double J[3][3];
      for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) J[i][k] = (dR[k][3 * i] * gc[0] + dR[k][3 * i + 1] * gc[1]) + dR[k][3 * i + 2] * gc[2];
      const int row[3] = {22, 25, 27};  // H(3, 3), H(4, 4), H(5, 5)
      for (int a = 0; a < 3; ++a)
      {
        sums[4 + a] += w * ((J[0][a] * r0 + J[1][a] * r1) + J[2][a] * r2);
        for (int b = a; b < 3; ++b) sums[row[a] + (b - a)] += w * ((J[0][a] * J[0][b] + J[1][a] * J[1][b]) + J[2][a] * J[2][b]);
      }
    }
  }
}

}  // namespace lsa
