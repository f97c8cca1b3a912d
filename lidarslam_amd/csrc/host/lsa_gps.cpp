// lsa_gps.cpp -- what surrounds a pose-graph solve with GPS position priors (lsa_pose_graph.h): which logged pose a fix belongs
// to, and the rigid transform that lays one track onto another, the solve's start.  Host only, no state; a stand-alone program
// links it (tests/pose_graph_prior_sanitize.cpp).
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../../include/lidarslam_amd.h"
#include "lsa_sym_eigen.h"

namespace
{
bool finite_d(double v) { return v - v == 0.; }

void quat_to_rot(const double* q, double* R)  // unit (w, x, y, z)
{
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1. - 2. * (y * y + z * z); R[1] = 2. * (x * y - w * z);      R[2] = 2. * (x * z + w * y);
  R[3] = 2. * (x * y + w * z);      R[4] = 1. - 2. * (x * x + z * z); R[5] = 2. * (y * z - w * x);
  R[6] = 2. * (x * z - w * y);      R[7] = 2. * (y * z + w * x);      R[8] = 1. - 2. * (x * x + y * y);
}

// the rotation of least angle that carries the direction of a onto that of b; the identity when one of them vanishes
void rot_between(const double* a, const double* b, double* R)
{
  const double na = std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), nb = std::sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
  double q[4] = {1., 0., 0., 0.};
  if (na > 0. && nb > 0. && finite_d(na) && finite_d(nb))
  {
    const double u[3] = {a[0] / na, a[1] / na, a[2] / na}, v[3] = {b[0] / nb, b[1] / nb, b[2] / nb};
    const double c = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    if (c > -1. + 1e-12)
    {
      q[0] = 1. + c;
      q[1] = u[1] * v[2] - u[2] * v[1];
      q[2] = u[2] * v[0] - u[0] * v[2];
      q[3] = u[0] * v[1] - u[1] * v[0];
    }
    else
    {
      // opposite directions: half a turn about an axis across u (the unit axis least along u, made orthogonal to it)
      int k = 0;
      for (int i = 1; i < 3; ++i)
        if (std::fabs(u[i]) < std::fabs(u[k])) k = i;
      double ax[3] = {0., 0., 0.};
      ax[k] = 1.;
      const double d = u[k];
      for (int i = 0; i < 3; ++i) ax[i] -= d * u[i];
      q[0] = 0.; q[1] = ax[0]; q[2] = ax[1]; q[3] = ax[2];
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) q[i] /= n;
  }
  quat_to_rot(q, R);
}
}  // namespace

extern "C" {

// Per fix, in order: among the logged poses, dated slam_times[j] + time_offset, the one nearest in time to the fix, if it is
// within max_time_diff (inclusive); of two equally near the earlier.  A fix whose pose is the pose of the fix accepted before
// it is dropped (-1), so that no pose is tied to two positions in a row.  Times ascending (LSA_E_ARG otherwise).
int lsa_gps_match_trajectory(const double* slam_times, int n, const double* gps_times, int G, double time_offset, double max_time_diff, int32_t* match_out)
{
  if (n < 0 || G < 0 || (n > 0 && !slam_times) || (G > 0 && (!gps_times || !match_out)) || !finite_d(time_offset) || !(max_time_diff >= 0.)) return LSA_E_ARG;
  std::vector<double> at(static_cast<size_t>(n));
  for (int j = 0; j < n; ++j)
  {
    at[static_cast<size_t>(j)] = slam_times[j] + time_offset;
    if (!finite_d(at[static_cast<size_t>(j)]) || (j > 0 && at[static_cast<size_t>(j)] < at[static_cast<size_t>(j) - 1])) return LSA_E_ARG;
  }
  for (int f = 0; f < G; ++f)
    if (!finite_d(gps_times[f])) return LSA_E_ARG;
  int previous = -1;
  for (int f = 0; f < G; ++f)
  {
    const double t = gps_times[f];
    int best = -1;
    if (n > 0)
    {
      const int hi = static_cast<int>(std::lower_bound(at.begin(), at.end(), t) - at.begin());  // the first pose not before the fix
      int lo = hi - 1;
      while (lo > 0 && at[static_cast<size_t>(lo) - 1] == at[static_cast<size_t>(lo)]) --lo;   // the earliest of equally dated poses
      const double dlo = lo >= 0 ? std::fabs(t - at[static_cast<size_t>(lo)]) : 0., dhi = hi < n ? std::fabs(t - at[static_cast<size_t>(hi)]) : 0.;
      if (lo >= 0 && (hi >= n || dlo <= dhi)) best = dlo <= max_time_diff ? lo : -1;
      else if (hi < n) best = dhi <= max_time_diff ? hi : -1;
    }
    if (best != -1 && best != previous)
    {
      previous = best;
      match_out[f] = best;
    }
    else
      match_out[f] = -1;
  }
  return LSA_OK;
}

// The rigid T (row-major 4x4) minimising sum |T from_i - to_i|^2 over the pairs: Horn's closed form -- the rotation is the
// eigenvector of the largest eigenvalue of the 4x4 symmetric N built from sum (from_i - mean)(to_i - mean)^T, the translation
// lays the means onto each other.  Fewer than three pairs, or the two largest eigenvalues within 1e-9 of the largest (collinear
// tracks: the rotation about the line is free): the reference's rough estimate (GlobalTrajectoriesRegistration.cxx:110-140),
// x -> R x + (to_0 - from_0) with R the least rotation carrying the chord from_last - from_0 onto to_last - to_0, the identity
// when a chord vanishes.
int lsa_trajectory_alignment(const double* from_xyz, const double* to_xyz, int pairs, double* T16_out)
{
  if (!from_xyz || !to_xyz || !T16_out || pairs < 1) return LSA_E_ARG;
  for (long long i = 0; i < 3LL * pairs; ++i)
    if (!finite_d(from_xyz[i]) || !finite_d(to_xyz[i])) return LSA_E_ARG;
  double R[9], t[3];
  bool closed = false;
  if (pairs >= 3)
  {
    double cf[3] = {0., 0., 0.}, ct[3] = {0., 0., 0.};
    for (int i = 0; i < pairs; ++i)
      for (int k = 0; k < 3; ++k) { cf[k] += from_xyz[3 * static_cast<size_t>(i) + k]; ct[k] += to_xyz[3 * static_cast<size_t>(i) + k]; }
    for (int k = 0; k < 3; ++k) { cf[k] /= pairs; ct[k] /= pairs; }
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < pairs; ++i)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) S[r * 3 + c] += (from_xyz[3 * static_cast<size_t>(i) + r] - cf[r]) * (to_xyz[3 * static_cast<size_t>(i) + c] - ct[c]);
    const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    const double N[16] = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
                          Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
                          Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
                          Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
    double ev[4], vec[16];
    lsa::host::SymEigen(4, N, ev, vec);
    if (finite_d(ev[3]) && ev[3] > 0. && ev[3] - ev[2] >= 1e-9 * ev[3])
    {
      double q[4] = {vec[3], vec[4 + 3], vec[8 + 3], vec[12 + 3]};
      const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      if (nq > 0.5)  // a unit vector to rounding
      {
        for (int k = 0; k < 4; ++k) q[k] /= nq;
        quat_to_rot(q, R);
        for (int k = 0; k < 3; ++k) t[k] = ct[k] - (R[k * 3] * cf[0] + R[k * 3 + 1] * cf[1] + R[k * 3 + 2] * cf[2]);
        closed = true;
      }
    }
  }
  if (!closed)
  {
    const double* f0 = from_xyz;
    const double* t0 = to_xyz;
    const double* f1 = from_xyz + 3 * static_cast<size_t>(pairs - 1);
    const double* t1 = to_xyz + 3 * static_cast<size_t>(pairs - 1);
    const double a[3] = {f1[0] - f0[0], f1[1] - f0[1], f1[2] - f0[2]}, b[3] = {t1[0] - t0[0], t1[1] - t0[1], t1[2] - t0[2]};
    rot_between(a, b, R);
    for (int k = 0; k < 3; ++k) t[k] = t0[k] - f0[k];
  }
  for (int r = 0; r < 3; ++r)
  {
    for (int c = 0; c < 3; ++c) T16_out[r * 4 + c] = R[r * 3 + c];
    T16_out[r * 4 + 3] = t[r];
  }
  T16_out[12] = 0.; T16_out[13] = 0.; T16_out[14] = 0.; T16_out[15] = 1.;
  return LSA_OK;
}

}  // extern "C"
