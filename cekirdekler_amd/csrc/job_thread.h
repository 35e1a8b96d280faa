// A worker's persistent host thread, which executes fan-out jobs (replacing
// Parallel.For, Cores.cs:747-834).  Pure host code.
#pragma once
#include <condition_variable>
#include <deque>
#include <exception>
#include <thread>

#include "common.h"

namespace cek {

class JobThread {
 public:
  // spin: both sides of the hand-off spin (with pause) for up to spin_us
  // before blocking on a condition variable: back-to-back computes (a loop of
  // enqueue-mode calls, ~10-20 µs apart) then cost an atomic store and a
  // cache-line transfer per device instead of a futex wake-up (tens of µs on
  // a busy host).  For GPU workers only: a CPU device's job runs on the CPU
  // pool, which needs every core the caller would spin on.
  // before_first_job: runs on the thread ahead of its first job (a GPU worker
  // makes its device current); when it throws, that job fails with its
  // exception and the next job tries again.
  JobThread(bool spin, std::function<void()> before_first_job);
  ~JobThread() { stop(); }
  JobThread(const JobThread&) = delete;
  JobThread& operator=(const JobThread&) = delete;

  void post(std::function<void()> fn);
  void wait();  // until every posted job ran; rethrows the first job exception
  void stop();  // runs what is still queued, then joins the thread
  static double spin_us;  // CEK_SPIN_US (default 50; 0: block at once)

 private:
  void loop();

  const bool spin_;
  const std::function<void()> before_first_job_;
  std::mutex mu_;  // guards q_, busy_, stop_, err_
  std::condition_variable cv_, idle_cv_;
  std::deque<std::function<void()>> q_;
  bool busy_ = false, stop_ = false;
  std::atomic<uint64_t> posted_{0}, finished_{0};  // jobs handed over / completed
  std::atomic<bool> sleeping_{false}, waiter_blocked_{false};
  std::exception_ptr err_;
  std::thread th_;  // last: started once everything above exists
};

}  // namespace cek
