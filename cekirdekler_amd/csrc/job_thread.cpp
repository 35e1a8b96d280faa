#include "job_thread.h"

namespace cek {

JobThread::JobThread(bool spin, std::function<void()> before_first_job)
    : spin_(spin), before_first_job_(std::move(before_first_job)), th_([this] { loop(); }) {}

void JobThread::stop() {
  {
    std::lock_guard<std::mutex> g(mu_);
    stop_ = true;
  }
  cv_.notify_all();
  if (th_.joinable()) th_.join();
}

static double env_spin_us() {
  const char* e = std::getenv("CEK_SPIN_US");
  return e ? std::max(0.0, std::atof(e)) : 50.0;
}
double JobThread::spin_us = env_spin_us();

static inline void cpu_relax() { __builtin_ia32_pause(); }

void JobThread::post(std::function<void()> fn) {
  {
    std::lock_guard<std::mutex> g(mu_);
    q_.push_back(std::move(fn));
    posted_.fetch_add(1, std::memory_order_release);
  }
  if (sleeping_.load(std::memory_order_acquire)) cv_.notify_one();
}

void JobThread::wait() {
  const uint64_t target = posted_.load(std::memory_order_acquire);
  if (finished_.load(std::memory_order_acquire) < target && spin_us > 0 && spin_) {
    const double until = now_ms() + spin_us * 1e-3;
    int n = 0;
    while (finished_.load(std::memory_order_acquire) < target) {
      cpu_relax();
      if ((++n & 63) == 0 && now_ms() > until) break;
    }
  }
  std::unique_lock<std::mutex> lk(mu_);
  if (finished_.load(std::memory_order_acquire) < target) {
    waiter_blocked_.store(true, std::memory_order_release);
    idle_cv_.wait(lk, [&] { return q_.empty() && !busy_; });
    waiter_blocked_.store(false, std::memory_order_release);
  }
  if (err_) {
    auto e = err_;
    err_ = nullptr;
    std::rethrow_exception(e);
  }
}

void JobThread::loop() {
  bool first_done = !before_first_job_;
  for (;;) {
    std::function<void()> job;
    // spin for new work first (a hot loop of computes posts every few µs)
    if (spin_us > 0 && !stop_ && spin_) {
      const uint64_t seen = finished_.load(std::memory_order_acquire);
      const double until = now_ms() + spin_us * 1e-3;
      int n = 0;
      while (posted_.load(std::memory_order_acquire) == seen) {
        cpu_relax();
        if ((++n & 63) == 0 && now_ms() > until) break;
      }
    }
    {
      std::unique_lock<std::mutex> lk(mu_);
      if (q_.empty() && !stop_) {
        sleeping_.store(true, std::memory_order_release);
        cv_.wait(lk, [&] { return stop_ || !q_.empty(); });
        sleeping_.store(false, std::memory_order_release);
      }
      if (stop_ && q_.empty()) return;
      job = std::move(q_.front());
      q_.pop_front();
      busy_ = true;
    }
    try {
      if (!first_done) {
        before_first_job_();
        first_done = true;
      }
      job();
    } catch (...) {
      std::lock_guard<std::mutex> g(mu_);
      if (!err_) err_ = std::current_exception();
    }
    {
      std::lock_guard<std::mutex> g(mu_);
      busy_ = false;
      finished_.fetch_add(1, std::memory_order_release);
    }
    if (waiter_blocked_.load(std::memory_order_acquire)) idle_cv_.notify_all();
  }
}

}  // namespace cek
