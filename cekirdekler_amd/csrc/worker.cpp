#include "worker.h"

#include <set>

#include "memory.h"

// hip/hip_ext.h declares this AMD launch (kernel start/stop events stamped by
// the dispatch) next to a template that needs the device-compiler headers;
// the host build takes the C declaration alone
extern "C" hipError_t hipExtModuleLaunchKernel(hipFunction_t f, uint32_t globalWorkSizeX, uint32_t globalWorkSizeY,
                                               uint32_t globalWorkSizeZ, uint32_t localWorkSizeX,
                                               uint32_t localWorkSizeY, uint32_t localWorkSizeZ,
                                               size_t sharedMemBytes, hipStream_t hStream, void** kernelParams,
                                               void** extra, hipEvent_t startEvent, hipEvent_t stopEvent,
                                               uint32_t flags);

namespace cek {

// Makes dev's GPU current in its sync mode; the worker's first member is built
// from the result, so every part below finds the device ready.
static const DeviceInfo& made_current(const DeviceInfo& dev) {
  if (dev.type == kGPU) {
    CEK_HIP(hipSetDevice(dev.ordinal));
    apply_sync_mode(dev.ordinal);
  }
  return dev;
}

Worker::Worker(const DeviceInfo& dev, std::shared_ptr<Program> prog, int index, int queue_concurrency,
               bool /*no_pipelining*/, int cpu_slot)
    : dev_(made_current(dev)), prog_(std::move(prog)), index_(index),
      lanes_(dev_, std::min(std::max(queue_concurrency, 1), 16)), replicas_(dev_), markers_(dev_, lanes_),
      stamps_(dev_),
      cpu_(gpu() ? nullptr : new CpuLauncher(dev_.cpu_threads > 0 ? dev_.cpu_threads : 1, cpu_slot)),
      jobs_(gpu(), gpu() ? std::function<void()>([this] { set_device(); }) : nullptr) {}

Worker::~Worker() {
  jobs_.stop();  // runs what is still queued
  if (!gpu()) return;
  try {  // nothing below is freed while the device still works on it
    set_device();
    sync_all();
  } catch (...) {
  }
}

// CEK_HIP_SYNC=blocking|yield|spin: how a host thread waits in stream and
// event synchronisation on this device (hipSetDeviceFlags).  The default
// leaves HIP's own choice.  A waiting thread that spins takes a CPU from a
// co-executing CPU device's share; "blocking" sleeps until the GPU signals.
void apply_sync_mode(int ordinal) {
  static const unsigned flags = [] {
    const char* e = std::getenv("CEK_HIP_SYNC");
    const std::string m = e ? e : "";
    if (m == "blocking") return static_cast<unsigned>(hipDeviceScheduleBlockingSync);
    if (m == "yield") return static_cast<unsigned>(hipDeviceScheduleYield);
    if (m == "spin") return static_cast<unsigned>(hipDeviceScheduleSpin);
    return 0u;
  }();
  if (!flags) return;
  static std::mutex mu;
  static std::set<int> done;
  std::lock_guard<std::mutex> g(mu);
  if (!done.insert(ordinal).second) return;
  if (hipSetDeviceFlags(flags) != hipSuccess) (void)hipGetLastError();  // too late for this device: keep HIP's mode
}

void Worker::set_device() const {
  if (gpu()) CEK_HIP(hipSetDevice(dev_.ordinal));
}

hipEvent_t Worker::event(int slot) {
  while (static_cast<int>(events_.size()) <= slot) {
    events_.emplace_back();
    events_.back().get(dev_);
  }
  return events_[slot].peek();
}

void Worker::wait_stream(hipStream_t s, bool sleep) {
  if (!gpu()) return;
  if (!sleep) {
    CEK_HIP(hipStreamSynchronize(s));
    return;
  }
  const hipEvent_t e = sleep_ev_.get(dev_, hipEventBlockingSync | hipEventDisableTiming);
  CEK_HIP(hipEventRecord(e, s));
  CEK_HIP(hipEventSynchronize(e));
}

void Worker::system_release(hipStream_t s) {
  if (!gpu()) return;
  CEK_HIP(hipEventRecord(sys_ev_.get(dev_, hipEventDisableTiming), s));  // system fence kept
}

void Worker::gate_all_streams(const uint32_t* word, uint32_t value) {
  if (!gpu()) return;
  set_device();
  void* dptr = host_device_ptr(const_cast<uint32_t*>(word));
  lanes_.for_each_opened([&](hipStream_t s) {
    CEK_HIP(hipStreamWaitValue32(s, dptr, value, hipStreamWaitValueGte, 0xffffffffu));
  });
}

void Worker::RepeatGraphs::clear() {
  for (auto& kv : execs) (void)hipGraphExecDestroy(kv.second);
  execs.clear();
}

void Worker::launch_graph(hipStream_t s, const std::string& key,
                          const std::function<void(hipStream_t)>& fn) {
  auto it = graphs_.execs.find(key);
  if (it == graphs_.execs.end()) {
    hipGraph_t g = nullptr;
    CEK_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    try {
      fn(s);
    } catch (...) {
      (void)hipStreamEndCapture(s, &g);
      if (g) (void)hipGraphDestroy(g);
      throw;
    }
    CEK_HIP(hipStreamEndCapture(s, &g));
    hipGraphExec_t ex = nullptr;
    hipError_t e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    CEK_HIP(e);
    if (graphs_.execs.size() >= 64) graphs_.clear();  // bounded cache: drop everything, recapture on demand
    it = graphs_.execs.emplace(key, ex).first;
  }
  CEK_HIP(hipGraphLaunch(it->second, s));
}

void Worker::h2d(hipStream_t s, const ArraySpec& a, uint64_t elem_begin, uint64_t elem_count) {
  if (!gpu() || a.zc || elem_count == 0) return;
  replicas_.check_capturable(a);
  uint64_t off = elem_begin * a.elem_size, n = elem_count * a.elem_size;
  if (off >= a.bytes) return;
  if (off + n > a.bytes) n = a.bytes - off;
  char* d = static_cast<char*>(buffer(a));
  CEK_HIP(hipMemcpyAsync(d + off, static_cast<const char*>(a.host) + off, n, hipMemcpyHostToDevice, s));
}

void Worker::d2h(hipStream_t s, const ArraySpec& a, uint64_t elem_begin, uint64_t elem_count) {
  if (!gpu() || a.zc || elem_count == 0) return;
  replicas_.check_capturable(a);
  uint64_t off = elem_begin * a.elem_size, n = elem_count * a.elem_size;
  if (off >= a.bytes) return;
  if (off + n > a.bytes) n = a.bytes - off;
  char* d = static_cast<char*>(buffer(a));
  if (kernel_d2h.load(std::memory_order_relaxed) && d2h_by_kernel(s, a.host, off, d + off, n)) return;
  CEK_HIP(hipMemcpyAsync(static_cast<char*>(a.host) + off, d + off, n, hipMemcpyDeviceToHost, s));
}

// 16 bytes per lane per iteration; a grid of at most 64 work-groups: PCIe
// (≈ 55 GB/s) is the limit, so the copy leaves the rest of the chip to the
// kernels it overlaps
static const char* kCopySrc = R"CEK(
typedef unsigned int cek_u32x4 __attribute__((ext_vector_type(4)));
__global__ void cek_copy16_to_host(const cek_u32x4* src, cek_u32x4* dst, long long n16) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n16; i += stride) dst[i] = src[i];
}
)CEK";

bool Worker::d2h_by_kernel(hipStream_t s, void* host_base, uint64_t off, const void* src_dev, uint64_t n) {
  char* dst_host = static_cast<char*>(host_base) + off;
  if (n < kKernelD2HMinBytes || (reinterpret_cast<uintptr_t>(dst_host) | reinterpret_cast<uintptr_t>(src_dev) | n) & 15)
    return false;
  if (!host_is_pinned(host_base)) return false;  // pinned / registered: looked up by the array's base
  set_device();
  char* base_dev = static_cast<char*>(host_device_ptr(host_base));
  if (!base_dev) return false;
  void* dst = base_dev + off;
  {
    std::lock_guard<std::mutex> g(copy_mu_);
    if (!copy_fn_) {
      copy_prog_ = Program::build(dev_, kCopySrc, {}, {});
      if (!copy_prog_->ok()) throw Error("kernel-D2H copy kernel failed to build: " + copy_prog_->log());
      copy_fn_ = copy_prog_->gpu_fn("cek_copy16_to_host");
    }
  }
  long long n16 = static_cast<long long>(n / 16), hidden_off = 0, gs = n16;
  const void* src = src_dev;
  void* params[] = {&src, &dst, &n16, &hidden_off, &gs};
  const long long per_group = 256ll * 16;  // 16 iterations of 256 lanes per work-group at least
  const unsigned groups = static_cast<unsigned>(std::max(1ll, std::min(64ll, (n16 + per_group - 1) / per_group)));
  CEK_HIP(hipModuleLaunchKernel(copy_fn_, groups, 1, 1, 256, 1, 1, 0, s, params, nullptr));
  kernel_d2h_bytes_ += n;
  return true;
}

void Worker::launch(hipStream_t s, const std::string& kernel, const std::vector<ArraySpec>& arrs,
                    long long offset, long long count, int local, long long gsize) {
  if (count <= 0) return;
  if (local <= 0) throw Error("local range must be positive");
  if (count % local != 0)
    throw Error("range " + std::to_string(count) + " is not a multiple of local range " +
                std::to_string(local));
  if (!gpu()) {
    std::vector<void*> ptrs(arrs.size());
    for (size_t i = 0; i < arrs.size(); ++i) ptrs[i] = arrs[i].host;
    cpu_->launch(prog_->cpu_fn(kernel), kernel, ptrs.data(), offset, count, local, gsize);
    return;
  }
  hipFunction_t f = prog_->gpu_fn(kernel);
  std::vector<void*> ptrs(arrs.size());
  for (size_t i = 0; i < arrs.size(); ++i) ptrs[i] = buffer(arrs[i]);
  long long off = offset, gs = gsize;
  const bool dyn = prog_->dynamic();
  void* q = dyn ? lanes_.enqueue_queue(s) : nullptr;
  int level = 0;
  std::vector<void*> params(arrs.size() + (dyn ? 4 : 2));
  for (size_t i = 0; i < arrs.size(); ++i) params[i] = &ptrs[i];
  params[arrs.size()] = &off;
  params[arrs.size() + 1] = &gs;
  if (dyn) {
    params[arrs.size() + 2] = &q;
    params[arrs.size() + 3] = &level;
    // fresh level counts for this parent (errors accumulate)
    CEK_HIP(hipMemsetAsync(q, 0, 8 * sizeof(int), s));
  }
  unsigned grid = static_cast<unsigned>(count / local);
  if (kernel_times_on.load(std::memory_order_relaxed)) {
    hipEvent_t a = stamps_.event(), b = stamps_.event();
    CEK_HIP(hipExtModuleLaunchKernel(f, grid * static_cast<unsigned>(local), 1, 1, static_cast<unsigned>(local),
                                     1, 1, dyn_lds_, s, params.data(), nullptr, a, b, 0));
    stamps_.push(kernel, a, b);
  } else {
    CEK_HIP(hipModuleLaunchKernel(f, grid, 1, 1, static_cast<unsigned>(local), 1, 1, dyn_lds_, s,
                                  params.data(), nullptr));
  }
  if (dyn && prog_->has_dispatcher(kernel)) {
    // one launch per child level, same stream: level L's records were
    // written by level L-1's kernel, which the stream has completed
    hipFunction_t d = prog_->gpu_fn("__cek_dispatch_" + kernel);
    const unsigned dgrid = static_cast<unsigned>(std::max(1, dev_.compute_units) * 4);
    for (int L = 1; L <= std::min(device_enqueue_levels, kDynLevels - 1); ++L) {
      level = L;
      CEK_HIP(hipModuleLaunchKernel(d, dgrid, 1, 1, 256, 1, 1, 0, s, params.data(), nullptr));
    }
  }
  if (debug_checks.load(std::memory_order_relaxed)) replicas_.check_guards(s, kernel, arrs);
}

int Worker::device_enqueue_errors() {
  if (!gpu() || lanes_.enqueue_queues().empty()) return 0;
  set_device();
  sync_all();
  int total = 0;
  for (auto& dq : lanes_.enqueue_queues()) {
    int e = 0;
    CEK_HIP(hipMemcpy(&e, static_cast<char*>(dq.second) + 8 * sizeof(int), sizeof(int), hipMemcpyDeviceToHost));
    total += e;
  }
  return total;
}

}  // namespace cek
