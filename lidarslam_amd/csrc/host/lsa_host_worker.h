// lsa_host_worker.h -- one persistent host thread that runs jobs in submission order.
#pragma once
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>

namespace lsa
{
namespace host
{

// Each map has one: the keyframe's insertion (RollingGrid::Add, hash-map bound) is handed to it at the end of AddFrame
// and overlaps the next frame's keypoint extraction and ego-motion ICP on the device, and the sub-maps of the three
// keypoint types are extracted side by side.  Wait() is called before anything else reads a map.
// Same operations in the same order on the same containers: results do not depend on the overlap.
class HostWorker
{
public:
  HostWorker();
  ~HostWorker();
  void Submit(std::function<void()> job);
  void Wait();
  // A job is about to be submitted (within `seconds`): the thread wakes up now and polls for it instead of sleeping, so that
  // the job starts within a microsecond of Submit instead of a scheduler's wake-up later (tens of microseconds on an idle
  // host, a fifth of a frame and more on a busy one: a map insertion enqueued late runs INTO the next frame's ICP kernels
  // instead of in front of them).  Costs the polling time on one core, bounded by `seconds`.
  void Expect(double seconds);

private:
  void Run();
  std::mutex M;
  std::condition_variable Cv, Idle;
  std::deque<std::function<void()>> Jobs;
  bool Busy = false, Quit = false;
  std::atomic<int> Posted{0};           // jobs in the queue (read without the lock by the polling thread)
  std::atomic<long long> PollUntil{0};  // steady-clock nanoseconds
  std::atomic<bool> Leaving{false};
  std::thread T;
};

}  // namespace host
}  // namespace lsa
