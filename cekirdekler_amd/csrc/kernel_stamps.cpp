#include "kernel_stamps.h"

namespace cek {

KernelStamps::~KernelStamps() {
  if (stamps_.empty() && spare_.empty()) return;
  (void)hipSetDevice(dev_.ordinal);
  for (auto& k : stamps_) {
    spare_.push_back(k.start);
    spare_.push_back(k.stop);
  }
  for (auto e : spare_) (void)hipEventDestroy(e);
}

hipEvent_t KernelStamps::event() {
  {
    std::lock_guard<std::mutex> g(mu_);
    if (!spare_.empty()) {
      hipEvent_t e = spare_.back();
      spare_.pop_back();
      return e;
    }
  }
  CEK_HIP(hipSetDevice(dev_.ordinal));
  hipEvent_t e = nullptr;
  CEK_HIP(hipEventCreate(&e));  // timing enabled
  return e;
}

void KernelStamps::push(const std::string& kernel, hipEvent_t start, hipEvent_t stop) {
  std::lock_guard<std::mutex> g(mu_);
  if (stamps_.size() >= kMax) {  // recording left on: keep the newest
    spare_.push_back(stamps_.front().start);
    spare_.push_back(stamps_.front().stop);
    stamps_.pop_front();
  }
  stamps_.push_back({kernel, start, stop});
}

std::vector<std::pair<std::string, double>> KernelStamps::drain() {
  std::deque<Stamp> st;
  {
    std::lock_guard<std::mutex> g(mu_);
    st.swap(stamps_);
  }
  std::vector<std::pair<std::string, double>> out;
  out.reserve(st.size());
  for (auto& k : st) {
    CEK_HIP(hipEventSynchronize(k.stop));
    float ms = 0.f;
    CEK_HIP(hipEventElapsedTime(&ms, k.start, k.stop));
    out.emplace_back(k.kernel, ms);
  }
  std::lock_guard<std::mutex> g(mu_);
  for (auto& k : st) {
    spare_.push_back(k.start);
    spare_.push_back(k.stop);
  }
  return out;
}

}  // namespace cek
