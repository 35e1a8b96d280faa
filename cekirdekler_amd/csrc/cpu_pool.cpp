#include "cpu_pool.h"

#include <unistd.h>

#include <map>

namespace cek {

// Pool threads alive in the process: spinning only pays while every spinner
// has a core (two CPU devices of one host would otherwise spin 2·(N-1)
// threads on N cores and starve each other).
// Off by default (CEK_POOL_SPIN_US): measured on an 8-vCPU VM, spinning pool
// threads made a tiny CPU-device compute 1.5-3x slower (20 -> 33-60 µs; two
// CPU devices 42-51 -> 130-141 µs), and under a cgroup CPU quota (the GPU
// boxes give a process a 16-CPU share of a much larger machine) every
// spinning thread burns the share the computing threads need.
static std::atomic<int> g_pool_threads{0};
static double env_pool_spin_us() {
  const char* e = std::getenv("CEK_POOL_SPIN_US");
  return e ? std::max(0.0, std::atof(e)) : 0.0;
}
static const double g_pool_spin_us = env_pool_spin_us();
static bool pool_may_spin() {
  static const int cores = std::max(1u, std::thread::hardware_concurrency());
  return g_pool_spin_us > 0 && g_pool_threads.load(std::memory_order_relaxed) < cores;
}

CpuPool::CpuPool(int threads) : pid_(static_cast<long>(getpid())) {
  for (int i = 1; i < threads; ++i) threads_.emplace_back([this] { loop(); });
  g_pool_threads += static_cast<int>(threads_.size());
}

CpuPool::~CpuPool() {
  {
    std::lock_guard<std::mutex> g(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  for (auto& t : threads_) t.join();
  g_pool_threads -= static_cast<int>(threads_.size());
}

static inline void pool_relax() { __builtin_ia32_pause(); }


void CpuPool::loop() {
  uint64_t seen = 0;
  for (;;) {
    if (pool_may_spin()) {  // a new generation usually follows within µs
      const double until = now_ms() + g_pool_spin_us * 1e-3;
      int k = 0;
      while (gen_.load(std::memory_order_acquire) == seen) {
        pool_relax();
        if ((++k & 63) == 0 && now_ms() > until) break;
      }
    }
    const std::function<void(long long)>* fn;
    long long n;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return stop_ || gen_.load(std::memory_order_relaxed) != seen; });
      if (stop_) return;
      seen = gen_.load(std::memory_order_relaxed);
      fn = fn_;
      n = n_;
      if (!fn) continue;
      active_.fetch_add(1, std::memory_order_acq_rel);
    }
    for (long long i = next_++; i < n; i = next_++) (*fn)(i);
    {
      std::lock_guard<std::mutex> g(mu_);
      active_.fetch_sub(1, std::memory_order_acq_rel);
    }
    done_cv_.notify_all();
  }
}

std::shared_ptr<CpuPool> CpuPool::shared(int threads, int slot) {
  static const bool on = [] {
    const char* e = std::getenv("CEK_SHARED_CPU_POOL");
    return !(e && std::string(e) == "0");
  }();
  threads = std::max(1, threads);
  if (!on) return std::make_shared<CpuPool>(threads);
  static std::mutex mu;
  static std::map<std::pair<int, int>, std::weak_ptr<CpuPool>> pools;
  std::lock_guard<std::mutex> g(mu);
  auto& w = pools[{threads, slot}];
  auto p = w.lock();
  // a pool inherited through fork() has no threads in this process
  if (p && p->pid_ != static_cast<long>(getpid())) p.reset();
  if (!p) {
    p = std::make_shared<CpuPool>(threads);
    w = p;
  }
  return p;
}

void CpuPool::parallel_for(long long n, const std::function<void(long long)>& fn) {
  if (n <= 0) return;
  if (threads_.empty() || n == 1) {
    for (long long i = 0; i < n; ++i) fn(i);
    return;
  }
  std::lock_guard<std::mutex> turn(call_mu_);
  {
    std::lock_guard<std::mutex> g(mu_);
    fn_ = &fn;
    n_ = n;
    next_ = 0;
    gen_.fetch_add(1, std::memory_order_release);
  }
  // wake only as many pool threads as there are items beyond the caller's
  // first (a small range need not wake the whole pool)
  if (n - 1 >= static_cast<long long>(threads_.size())) {
    cv_.notify_all();
  } else {
    for (long long k = 0; k < n - 1; ++k) cv_.notify_one();
  }
  for (long long i = next_++; i < n; i = next_++) fn(i);
  // every item is claimed; wait (spinning first) for the threads still running one
  if (pool_may_spin()) {
    const double until = now_ms() + g_pool_spin_us * 1e-3;
    int k = 0;
    while (active_.load(std::memory_order_acquire) != 0) {
      pool_relax();
      if ((++k & 63) == 0 && now_ms() > until) break;
    }
  }
  std::unique_lock<std::mutex> lk(mu_);
  done_cv_.wait(lk, [&] { return active_.load(std::memory_order_acquire) == 0 && next_ >= n; });
  fn_ = nullptr;
}

void CpuLauncher::launch(CpuRunner fn, const std::string& kernel, void** argv, long long offset, long long count,
                         int local, long long gsize) {
  long long groups = count / local;
  // chunk groups so every pool thread gets several (amortise dispatch);
  // size() already counts the caller, so nthreads + 1 over-counts by one
  // (CpuPool thread count): kept as it is
  long long nthreads = pool_->size();
  long long tasks_max = std::max<long long>(1, std::min(groups, (nthreads + 1) * 8));
  // ...but no task shorter than kCpuMinTaskNs by this kernel's measured
  // cost per work item: a small range (the CPU's share of a GPU+CPU wave
  // frame is ~1,400 vertices) runs on the calling thread alone instead of
  // paying every pool thread's wake-up
  double& est = item_ns_[kernel];
  if (est > 0) {
    const double by_work = est * static_cast<double>(count) / kCpuMinTaskNs;
    tasks_max = std::max<long long>(1, std::min<long long>(tasks_max, static_cast<long long>(by_work)));
  }
  const long long per = (groups + tasks_max - 1) / tasks_max;
  const long long tasks = (groups + per - 1) / per;
  const double t0 = now_ms();
  pool_->parallel_for(tasks, [&](long long t) {
    long long g0 = t * per, g1 = std::min(groups, g0 + per);
    fn(argv, offset, gsize, offset + g0 * local, (g1 - g0) * local, local);
  });
  // per-item cost on one thread: wall time × the threads that ran
  const double used = static_cast<double>(std::min<long long>(tasks, nthreads + 1));
  const double ns = (now_ms() - t0) * 1e6 * used / static_cast<double>(std::max<long long>(1, count));
  est = est > 0 ? 0.7 * est + 0.3 * ns : ns;
}

}  // namespace cek
