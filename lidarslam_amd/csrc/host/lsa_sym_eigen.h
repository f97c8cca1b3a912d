// lsa_sym_eigen.h -- the cyclic Jacobi eigen-decomposition of a small symmetric matrix, for the units of the host that need one:
// the LM solve's degeneracy analysis (lsa_lm.cpp) and Horn's closed-form alignment of two tracks (lsa_gps.cpp).
#pragma once
#include <algorithm>
#include <cmath>

namespace lsa
{
namespace host
{
// cyclic Jacobi eigen-decomposition of a small symmetric matrix; ascending eigenvalues
inline void SymEigen(int n, const double* Ain, double* evals, double* evecs)
{
  double A[36], V[36];
  for (int i = 0; i < n * n; ++i) A[i] = Ain[i];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * n + j] = (i == j);
  // squared Frobenius norm: what the off-diagonal part is held against.  (The first version swept until that part was below
  // 1e-300 -- in practice until it had underflowed: twenty microseconds per frame for digits nobody can see.)
  double scale = 0;
  for (int i = 0; i < n * n; ++i) scale += A[i] * A[i];
  for (int sweep = 0; sweep < 100; ++sweep)
  {
    double off = 0;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
    if (off <= 1e-36 * scale) break;  // (machine precision is 5e-32 of the squared norm; Jacobi converges quadratically: one more sweep past it)
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q)
      {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::abs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k)
        {
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k)
        {
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k)
        {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  int order[6];
  for (int i = 0; i < n; ++i) order[i] = i;
  std::sort(order, order + n, [&](int a, int b) { return A[a * n + a] < A[b * n + b]; });
  for (int i = 0; i < n; ++i)
  {
    evals[i] = A[order[i] * n + order[i]];
    for (int k = 0; k < n; ++k) evecs[k * n + i] = V[k * n + order[i]];
  }
}
}  // namespace host
}  // namespace lsa
