// lsa_host_worker.cpp -- see lsa_host_worker.h.
#include "lsa_host_worker.h"
#include <chrono>

namespace lsa
{
namespace host
{
static long long SteadyNs() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
HostWorker::HostWorker() : T([this] { Run(); }) {}
HostWorker::~HostWorker()
{
  {
    std::lock_guard<std::mutex> l(M);
    Quit = true;
    Leaving.store(true);
  }
  Cv.notify_all();
  T.join();
}
void HostWorker::Submit(std::function<void()> job)
{
  {
    std::lock_guard<std::mutex> l(M);
    Jobs.push_back(std::move(job));
    Posted.fetch_add(1, std::memory_order_release);
  }
  Cv.notify_one();
}
void HostWorker::Expect(double seconds)
{
  PollUntil.store(SteadyNs() + static_cast<long long>(seconds * 1e9), std::memory_order_release);
  Cv.notify_one();
}
void HostWorker::Wait()
{
  std::unique_lock<std::mutex> l(M);
  Idle.wait(l, [this] { return Jobs.empty() && !Busy; });
}
void HostWorker::Run()
{
  std::unique_lock<std::mutex> l(M);
  while (true)
  {
    Cv.wait(l, [this] { return Quit || !Jobs.empty() || SteadyNs() < PollUntil.load(std::memory_order_acquire); });
    if (Jobs.empty())
    {
      if (Quit) return;  // nothing left to do
      // woken ahead of a job (Expect): poll for it, without the lock, until it is there or the time is up
      l.unlock();
      while (Posted.load(std::memory_order_acquire) == 0 && !Leaving.load() && SteadyNs() < PollUntil.load(std::memory_order_acquire))
      {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
      PollUntil.store(0, std::memory_order_release);
      l.lock();
      continue;
    }
    std::function<void()> job = std::move(Jobs.front());
    Jobs.pop_front();
    Posted.fetch_sub(1, std::memory_order_release);
    Busy = true;
    l.unlock();
    job();
    l.lock();
    Busy = false;
    if (Jobs.empty()) Idle.notify_all();
  }
}

}  // namespace host
}  // namespace lsa
