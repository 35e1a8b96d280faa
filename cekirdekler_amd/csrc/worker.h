// Per-device worker: the MI355X-native counterpart of the reference's
// ClObject.Worker (Worker.cs:33-1738).  A worker owns one device and the
// compiled program, and is made of parts that own their state and free it
// themselves: a lazily created table of HIP streams (LaneTable: main, up to 16
// round-robin compute streams, and read/compute/write streams for the two
// event-pipeline halves — the reference's 20-21 OpenCL queues,
// Worker.cs:75-259), one full-length device replica per host array (Replicas,
// Worker.cs:576-720), markers for fine-grained queue control (Markers), kernel
// timestamps (KernelStamps), and a persistent host thread that executes
// fan-out jobs (JobThread, replacing Parallel.For, Cores.cs:747-834).  The
// worker itself keeps the copies, the GPU launch and the repeat-graph cache.
//
// The CPU device executes the same kernel source compiled for the host on a
// thread pool (CpuLauncher); it works directly on host memory (no copies).
#pragma once
#include <unordered_map>

#include "common.h"
#include "cpu_pool.h"
#include "device.h"
#include "events.h"
#include "jit.h"
#include "job_thread.h"
#include "kernel_stamps.h"
#include "lanes.h"
#include "markers.h"
#include "replicas.h"

namespace cek {

// How host threads wait for GPU `ordinal` (env CEK_HIP_SYNC, worker.cpp).
void apply_sync_mode(int ordinal);

class Worker {
 public:
  // index: this worker's place among its Cores' workers
  // cpu_slot: this CPU device's index among the CPU devices of its set
  // (CpuPool::shared); ignored for a GPU
  Worker(const DeviceInfo& dev, std::shared_ptr<Program> prog, int index, int queue_concurrency,
         bool no_pipelining, int cpu_slot = 0);
  ~Worker();

  const DeviceInfo& dev() const { return dev_; }
  int index() const { return index_; }
  bool gpu() const { return dev_.type == kGPU; }
  uintptr_t cpu_pool_id() const { return reinterpret_cast<uintptr_t>(cpu_ ? cpu_->pool() : nullptr); }
  Program& program() { return *prog_; }

  // --- buffers (Replicas) ------------------------------------------------
  void* buffer(const ArraySpec& a) { return replicas_.buffer(a, debug_checks.load(std::memory_order_relaxed)); }
  // graph capture: while a log is set, every (uid, pointer) handed out is
  // appended to it; buffer_is() tells whether uid still has that pointer
  void set_capture_log(std::vector<std::pair<uint64_t, void*>>* log) { replicas_.set_capture_log(log); }
  bool buffer_is(uint64_t uid, const void* ptr) { return replicas_.buffer_is(uid, ptr); }
  void release(uint64_t uid) { replicas_.release(uid); }
  void release_all() { replicas_.release_all(); }
  uint64_t bytes_allocated() const { return replicas_.bytes_allocated(); }

  // --- streams (LaneTable) -----------------------------------------------
  hipStream_t main_stream() { return lanes_.open(main_lane_id()); }
  hipStream_t compute_stream(int i) { return lanes_.open(compute_lane_id(i % 16)); }  // i in [0, queue_concurrency)
  hipStream_t pipe_stream(int half, int role) { return lanes_.open(pipe_lane_id(half & 1, role % 3)); }
  // the same streams with their logical ids; compute_lane(q).id stays 1 + q
  // when one queue (queue_concurrency 1) aliases the stream to main
  Lane main_lane() { return {main_stream(), main_lane_id()}; }
  Lane compute_lane(int q) { return {compute_stream(q), compute_lane_id(q)}; }
  Lane pipe_lane(int half, int role) { return {pipe_stream(half, role), pipe_lane_id(half, role)}; }
  // Reserve `n` CUs (spread evenly over the XCDs) for copy kernels: the
  // pipeline's write streams run on those CUs only and every other stream
  // on the rest (CU-masked streams, LaneTable).  A download by copy kernel
  // (kernel_d2h) then never waits for a GEMM work-group to leave a CU, so
  // it runs beside the SDMA uploads (PCIe full duplex).  0: no masks.
  // Drains and re-creates the worker's streams.
  void set_cu_reserve(int n) { lanes_.set_cu_reserve(n); }
  int cu_reserve() const { return lanes_.cu_reserve(); }
  int next_compute_queue() { return rr_.fetch_add(1) % lanes_.queue_concurrency(); }  // round robin (Worker.cs:435-458)
  int queue_concurrency() const { return lanes_.queue_concurrency(); }
  hipEvent_t event(int slot);               // pooled, timing disabled
  // wait until stream s is idle: hipStreamSynchronize, or (sleep) a
  // blocking-sync event the host thread sleeps on
  void wait_stream(hipStream_t s, bool sleep);
  // `target` waits for everything queued so far on every other stream of
  // this worker (compute queues and pipeline streams): a copy issued next on
  // `target` neither overtakes a kernel still reading its destination nor
  // reads a source a kernel is still writing
  void join_streams(hipStream_t target) { lanes_.join(target); }
  // A marker with a SYSTEM-scope release on s (a default-flag event): stores
  // that kernels made straight into host memory (zero-copy arrays) are
  // visible to the host once s is synchronised, independent of the
  // fence-free timing events around them
  void system_release(hipStream_t s);
  void sync_all() { lanes_.sync_all(); }    // finish every created stream
  void set_device() const;

  // --- ops (enqueue on GPU; synchronous on the CPU device) --------------
  void h2d(hipStream_t s, const ArraySpec& a, uint64_t elem_begin, uint64_t elem_count);
  void d2h(hipStream_t s, const ArraySpec& a, uint64_t elem_begin, uint64_t elem_count);
  void launch(hipStream_t s, const std::string& kernel, const std::vector<ArraySpec>& arrs,
              long long offset, long long count, int local, long long gsize);
  void set_dynamic_lds(unsigned bytes) { dyn_lds_ = bytes; }
  // Device-side enqueue: child levels run after each parent launch (1..3)
  // and errors counted on the device (queue level full / too deep).
  int device_enqueue_levels = kDynLevels - 1;
  // Debug checks (Replicas): buffers allocated while on get a guard tail;
  // every launch is then synchronised and the guards of its arrays verified.
  // atomic: Cores::set_debug_checks flips it while job threads read it
  std::atomic<bool> debug_checks{false};
  // D2H of pinned / registered host memory by a copy kernel on the stream
  // (device writes straight into the host pages) instead of
  // hipMemcpyAsync, for copies of at least kKernelD2HMinBytes with 16-byte
  // aligned ends: keeps downloads off the SDMA rings the uploads use, so a
  // download gated on a kernel never blocks an upload queued behind it
  std::atomic<bool> kernel_d2h{false};
  // Kernel profiling timestamps (KernelStamps): while on, every launch goes
  // through hipExtModuleLaunchKernel with a start and a stop event that the
  // runtime stamps from the dispatch itself — the kernel's own execution
  // time, without the gap between back-to-back launches that stream events or
  // a host clock include.  kernel_times() drains them: (kernel, ms) in launch order.
  std::atomic<bool> kernel_times_on{false};
  std::vector<std::pair<std::string, double>> kernel_times() { return stamps_.drain(); }
  static constexpr uint64_t kKernelD2HMinBytes = 1ull << 20;
  uint64_t kernel_d2h_bytes() const { return kernel_d2h_bytes_; }
  int device_enqueue_errors();

  // --- markers (Markers) --------------------------------------------------
  void add_marker(hipStream_t s, bool release = false) { markers_.add(s, release); }
  // a device pool coalesces the markers of consecutive tasks: one
  // hipEventRecord per batch instead of per task
  void defer_marker(hipStream_t s, bool release = false) { markers_.defer(s, release); }
  void flush_markers() { markers_.flush(); }
  bool has_deferred_markers() const { return markers_.has_deferred(); }
  long long markers_reached() { return markers_.reached(); }
  std::pair<int, uint64_t> last_marker() const { return markers_.last(); }
  uint64_t marker_word(int slot) { return markers_.word(slot); }
  long long markers_issued() const { return markers_.issued(); }

  // --- user-event gating (ClUserEvent.cs:102-117) -------------------------
  // Every stream of this worker (created on demand) waits until *word >= value.
  void gate_all_streams(const uint32_t* word, uint32_t value);

  // --- graph replay of a repeat loop (hipGraph instead of N launches) ------
  // Launches `fn`'s stream work on `s`; the first call with `key` captures
  // it into a hipGraph, later calls replay the instantiated graph.
  void launch_graph(hipStream_t s, const std::string& key, const std::function<void(hipStream_t)>& fn);
  size_t graphs_cached() const { return graphs_.execs.size(); }

  // --- job thread (JobThread) ----------------------------------------------
  void post(std::function<void()> fn) { jobs_.post(std::move(fn)); }
  void wait() { jobs_.wait(); }  // rethrows the first job exception

 private:
  bool d2h_by_kernel(hipStream_t s, void* host_base, uint64_t off, const void* src_dev, uint64_t n);
  // the instantiated repeat graphs, at most 64
  struct RepeatGraphs {
    std::unordered_map<std::string, hipGraphExec_t> execs;
    void clear();
    ~RepeatGraphs() { clear(); }
  };

  // Declared in the order that makes destruction correct: ~Worker stops the
  // job thread and drains the device; then the members go last to first, so
  // the job thread before anything its jobs use, graphs, events and buffers
  // before the streams they were used on, and all of them before dev_.
  const DeviceInfo dev_;  // its GPU is current, in its sync mode, before any part is built
  std::shared_ptr<Program> prog_;
  const int index_;
  unsigned dyn_lds_ = 0;
  LaneTable lanes_;
  std::atomic<int> rr_{0};
  Replicas replicas_;
  std::vector<Event> events_;  // event(slot)
  Event sleep_ev_;             // wait_stream
  Event sys_ev_;               // system_release
  Markers markers_;
  KernelStamps stamps_;
  RepeatGraphs graphs_;
  std::shared_ptr<Program> copy_prog_;  // the kernel-D2H copy kernel, built on first use
  hipFunction_t copy_fn_ = nullptr;
  std::mutex copy_mu_;  // guards the two above
  std::atomic<uint64_t> kernel_d2h_bytes_{0};
  std::unique_ptr<CpuLauncher> cpu_;  // CPU device only
  JobThread jobs_;
};

// The scheduler's workers as its parts see them: each part is given a
// reference at construction and is destroyed before them.
using Workers = std::vector<std::unique_ptr<Worker>>;

}  // namespace cek
