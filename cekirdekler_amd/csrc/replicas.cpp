#include "replicas.h"

#include "memory.h"

namespace cek {

void* Replicas::buffer(const ArraySpec& a, bool checks) {
  void* p = find_or_allocate(a, checks);
  std::lock_guard<std::mutex> g(mu_);
  if (cap_log_) cap_log_->emplace_back(a.uid, p);
  return p;
}

void Replicas::set_capture_log(std::vector<std::pair<uint64_t, void*>>* log) {
  std::lock_guard<std::mutex> g(mu_);
  cap_log_ = log;
}

// A copy captured into a graph replays against the host pages it was
// captured with; from pageable memory the runtime would stage it through a
// bounce buffer at capture time, so the replay would not read (or write) the
// array's current contents.  Only pinned / registered host memory may be
// captured.
void Replicas::check_capturable(const ArraySpec& a) {
  {
    std::lock_guard<std::mutex> g(mu_);
    if (!cap_log_) return;
  }
  if (!host_is_pinned(a.host))
    throw Error("graph capture: array " + std::to_string(a.uid) + " (" + std::to_string(a.bytes) +
                " bytes) is pageable host memory; a captured copy needs pinned or registered memory "
                "(use a FastArr-backed ClArray, or set ClArray.auto_pin_min_bytes below its size)");
}

bool Replicas::buffer_is(uint64_t uid, const void* ptr) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = map_.find(uid);
  if (it == map_.end()) return false;
  if (it->second.ptr) return it->second.ptr == ptr;
  return it->second.zc && it->second.zc == ptr;
}

void* Replicas::find_or_allocate(const ArraySpec& a, bool checks) {
  if (dev_.type != kGPU) return a.host;
  if (a.zc) {
    // The array owns its registration (ClArray registers once, unregisters
    // on dispose); registering here per launch would leak refcounts and leave
    // a stale mapping behind once the host memory is freed.
    if (!host_is_pinned(a.host))
      throw Error("zero-copy array is neither pinned nor registered with HIP");
    std::lock_guard<std::mutex> g(mu_);
    return map_[a.uid].zc = host_device_ptr(a.host);
  }
  std::lock_guard<std::mutex> g(mu_);
  Replica& r = map_[a.uid];
  void* keep = nullptr;  // old replica whose contents move into a guarded one
  uint64_t keep_bytes = 0;
  if (r.ptr) {
    void* d = r.ptr;
    const uint64_t cap = r.bytes;
    if (cap >= a.bytes) {
      if (!checks) return d;
      if (r.guarded && r.guard_at == a.bytes) return d;
      // Debug checks need the guard right at the current extent: re-stamp it
      // there when the allocation has room (a guarded buffer reused at a
      // smaller size has), else move the contents into a guarded allocation.
      const uint64_t room = r.guarded ? r.guard_at + kGuardBytes : cap;
      if (room >= a.bytes + kGuardBytes) {
        CEK_HIP(hipSetDevice(dev_.ordinal));
        CEK_HIP(hipMemset(static_cast<char*>(d) + a.bytes, kGuardByte, kGuardBytes));
        r.guarded = true;
        r.guard_at = a.bytes;
        return d;
      }
      keep = d;
      keep_bytes = std::min<uint64_t>(cap, a.bytes);
    } else {
      (void)hipFree(d);
    }
    bytes_allocated_ -= cap;
    r.ptr = nullptr;
    r.bytes = 0;
    r.guarded = false;
  }
  void* d = nullptr;
  CEK_HIP(hipSetDevice(dev_.ordinal));
  const size_t guard = checks ? kGuardBytes : 0;
  hipError_t e = hipMalloc(&d, (a.bytes ? a.bytes : 1) + guard);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    throw Error("hipMalloc of " + std::to_string(a.bytes) + " bytes failed on " + dev_.name);
  }
  if (keep) {
    CEK_HIP(hipMemcpy(d, keep, keep_bytes, hipMemcpyDeviceToDevice));
    (void)hipFree(keep);
  }
  if (guard) {
    CEK_HIP(hipMemset(static_cast<char*>(d) + a.bytes, kGuardByte, guard));
    r.guarded = true;
    r.guard_at = a.bytes;
  }
  r.ptr = d;
  r.bytes = a.bytes;
  bytes_allocated_ += a.bytes;
  return d;
}

void Replicas::release(uint64_t uid) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = map_.find(uid);
  if (it == map_.end()) return;
  if (it->second.ptr) {
    CEK_HIP(hipSetDevice(dev_.ordinal));
    (void)hipFree(it->second.ptr);
    bytes_allocated_ -= it->second.bytes;
  }
  map_.erase(it);
}

void Replicas::release_all() {
  std::lock_guard<std::mutex> g(mu_);
  if (dev_.type == kGPU) {
    (void)hipSetDevice(dev_.ordinal);
    for (auto& kv : map_)
      if (kv.second.ptr) (void)hipFree(kv.second.ptr);
  }
  map_.clear();
  bytes_allocated_ = 0;
}

void Replicas::check_guards(hipStream_t s, const std::string& kernel, const std::vector<ArraySpec>& arrs) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return;  // graph replay
  hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    throw Error("kernel '" + kernel + "' failed on " + dev_.name + ": " + hipGetErrorString(e));
  }
  std::vector<unsigned char> tail(kGuardBytes);
  for (size_t i = 0; i < arrs.size(); ++i) {
    void* d = nullptr;
    uint64_t at = 0;
    {
      std::lock_guard<std::mutex> g(mu_);
      auto it = map_.find(arrs[i].uid);
      if (it == map_.end() || !it->second.ptr || !it->second.guarded) continue;
      d = it->second.ptr;
      at = it->second.guard_at;
    }
    CEK_HIP(hipMemcpy(tail.data(), static_cast<char*>(d) + at, kGuardBytes, hipMemcpyDeviceToHost));
    size_t bad = 0, first = kGuardBytes;
    for (size_t b = 0; b < kGuardBytes; ++b)
      if (tail[b] != kGuardByte) {
        ++bad;
        if (first == kGuardBytes) first = b;
      }
    if (bad) {
      CEK_HIP(hipMemset(static_cast<char*>(d) + at, kGuardByte, kGuardBytes));
      throw Error("kernel '" + kernel + "' wrote past the end of array #" + std::to_string(i) + " (" +
                  std::to_string(at) + " bytes) on " + dev_.name + ": " + std::to_string(bad) +
                  " guard bytes changed, first at +" + std::to_string(first));
    }
  }
}

}  // namespace cek
