// The CPU device's execution side: a host thread pool (the reference's CPU
// fission to N-1 cores, ClDevice.cs:85-95) and the rule that cuts a kernel
// launch into pool tasks.
#pragma once
#include <condition_variable>
#include <thread>
#include <unordered_map>

#include "common.h"
#include "jit.h"

namespace cek {

class CpuPool {
 public:
  explicit CpuPool(int threads);
  ~CpuPool();
  // Run fn(i) for i in [0, n) across the pool; blocks until done.  Callers
  // on different threads take turns (a pool may be shared, see shared()).
  void parallel_for(long long n, const std::function<void(long long)>& fn);
  int size() const { return static_cast<int>(threads_.size()) + 1; }
  // The process-wide pool of `threads` threads for the `slot`-th CPU device
  // of a device set: every cruncher's first CPU device of a given size runs
  // on the same threads, as an OpenCL CPU runtime shares one thread pool
  // among its contexts.  Separate crunchers on one host then see the same
  // CPU device (on a shared host a pool's speed depends on where its
  // threads landed: 3.0-4.4 ms for the same stream in four crunchers of one
  // process, profiles/r6/README.md) and do not oversubscribe the host when
  // used in turn; two CPU devices of ONE set (slots 0 and 1) still run side
  // by side.  CEK_SHARED_CPU_POOL=0: a pool per device.
  static std::shared_ptr<CpuPool> shared(int threads, int slot);

 private:
  void loop();
  long pid_ = 0;  // the process that started the threads (a forked child has none of them)
  std::mutex call_mu_;  // one parallel_for at a time
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(long long)>* fn_ = nullptr;
  long long n_ = 0;
  std::atomic<long long> next_{0};
  std::atomic<int> active_{0};
  // generation of the current parallel_for: pool threads may spin on it for
  // CEK_POOL_SPIN_US (default 0) before sleeping on cv_ (a frame loop calls
  // parallel_for every few tens of µs; a futex wake per thread per call
  // was the CPU device's fixed cost)
  std::atomic<uint64_t> gen_{0};
  bool stop_ = false;
};

// One CPU device's launches: its pool and, per kernel, the measured cost of a
// work item, from which a launch is cut into tasks worth a pool thread's
// wake-up.
class CpuLauncher {
 public:
  CpuLauncher(int threads, int slot) : pool_(CpuPool::shared(threads, slot)) {}
  // Runs `count` work items from `offset` in groups of `local`; blocks until done.
  void launch(CpuRunner fn, const std::string& kernel, void** argv, long long offset, long long count,
              int local, long long gsize);
  const CpuPool* pool() const { return pool_.get(); }

 private:
  std::shared_ptr<CpuPool> pool_;
  // measured ns per work item per kernel (one thread), and the shortest task
  // worth handing to a pool thread
  std::unordered_map<std::string, double> item_ns_;
  static constexpr double kCpuMinTaskNs = 20000.0;
};

}  // namespace cek
