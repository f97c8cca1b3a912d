// lsa_slam_internal.h -- what every unit of SlamCore (lsa_slam_*.cpp) uses and nobody else: the stage timers' clock, the
// stamp conversion, the early return on a failed call into the C ABI.
#pragma once
#include <chrono>
#include <cstdint>
#include "lsa_slam_core.h"

namespace lsa
{
namespace host
{
namespace
{
struct Tick
{
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  double Stop() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
};
inline double StampToSec(uint64_t us) { return us * 1e-6; }  // Utils::PclStampToSec
// the extractor every LiDAR device starts from
inline lsa_extract_params_t DefaultExtractParams()
{
  return lsa_extract_params_t{4, 1.5f, 10.f, 0.5f, 0.86f, 0.20f, 0.15f, 1.5f, 50.f};  // SSKE.h:125-148
}
}  // namespace

#define LSA_TRY(call)                          \
  do                                           \
  {                                            \
    int rc__ = (call);                         \
    if (rc__ < 0) return Fail(rc__, #call);    \
  } while (0)

}  // namespace host
}  // namespace lsa
