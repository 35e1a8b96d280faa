// Multi-device scheduler — the MI355X-native counterpart of the reference's
// `Cores` (Cores.cs:37-1982): one worker per device, per-compute-id range
// tables driven by the iterative load balancer, and three execution shapes
// per device:
//   * 3-phase (H2D → kernels → D2H) on one in-order stream
//     (Cores.cs:745-835, Worker.cs:821-840/:1033-1114/:1343-1361),
//   * event-driven pipeline: the device's range cut into `blobs` chunks that
//     stream through two half-pipelines, each {read, compute, write} HIP
//     streams joined by hipEvents (Cores.cs:1197-1367, Worker.cs:1411-1567),
//   * driver pipeline: chunk k on round-robin stream k mod Q (Q = queue
//     concurrency, by default the GPU_MAX_HW_QUEUES hardware queues)
//     (Cores.cs:1368-1958).
// plus enqueue mode / async enqueue / no-compute / fine-grained markers /
// repeat + sync kernel (ClNumberCruncher.cs:66-187, Cores.cs:72-126,
// :449, :796-809).  Fan-out runs on persistent worker threads with the GIL
// released, one Python→C++ crossing per compute().
//
// Distributed mode (one process per GPU): the balancer runs on the global
// device list; each rank executes its own device's range and the per-device
// times are exchanged through an Exchanger, so every rank derives the
// identical next split.  Optional RCCL data plane: broadcast `read` arrays
// from rank 0 and all-gather written slices into every replica.
//
// Cores is the scheduler: balancer state, mode switches, compute() with its
// failover (cores.cpp) and the three execution shapes (cores_run.cpp).  Spans
// and timeline (spans.h), peer traffic (peer.h), compute graphs (graphs.h),
// deferred downloads (downloads.h), the schedule log (sched_log.h) and the
// shell GEMM's dims (shell_gemm.h) are parts that own and free their state.
#pragma once
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>

#include "balancer.h"
#include "dist.h"
#include "downloads.h"
#include "graphs.h"
#include "peer.h"
#include "sched_log.h"
#include "shell_gemm.h"
#include "spans.h"
#include "worker.h"

namespace cek {

struct ComputeCall {
  std::vector<std::string> kernels;
  int repeats = 1;
  std::string repeat_kernel;
  std::vector<ArraySpec> arrays;
  long long global_range = 0;
  long long local_range = 256;
  long long global_offset = 0;
  int compute_id = 1;
  bool pipeline = false;
  bool pipeline_event = true;  // PIPELINE_EVENT=true, PIPELINE_DRIVER=false
  int blobs = 4;
  // Split granularity in work items (0 = local range): every device range is
  // a multiple of it, e.g. to keep the K-split work-groups of one GEMM tile
  // on the same device.  Must be a multiple of local_range.
  long long granularity = 0;
  // Explicit, possibly uneven pipeline blobs (event pipeline, one device
  // holding the whole range): blob k = work items [blob_bounds[k],
  // blob_bounds[k+1]) of the range; blobs alternate between the two
  // half-pipelines.  Arrays may carry per-blob slices (ArraySpec::blob_begin).
  std::vector<long long> blob_bounds;
};

struct CoresConfig {
  int queue_concurrency = 16;
  bool no_pipelining = false;
  bool smooth = true;
  std::vector<std::string> options;
  std::vector<std::string> prebuilt;  // "path|name1,name2"
};

struct ComputeRecord {  // structured per-call record (observability)
  int compute_id = 0;
  double wall_ms = 0;
  std::vector<long long> ranges, references;
  std::vector<double> device_ms;
  uint64_t h2d_bytes = 0, d2h_bytes = 0;
  uint64_t p2p_bytes = 0;     // device→device bytes (read fan-out + keep-resident gather)
  uint64_t gather_bytes = 0;  // of which the keep-resident gather
  uint64_t staged_bytes = 0;  // of p2p_bytes: between GPUs without peer access (host-bounced)
  // where this call's device→device bytes went: "none" (no such copy),
  // "local" (logical devices of one GPU), "xgmi" (peer copies between GPUs),
  // "staged" (some pair without peer access), "pcie" (the read fan-out fell
  // back to one PCIe upload per device because a pair cannot peer)
  std::string p2p_path = "none";
  bool pipelined = false;
};

// Host-triggered event gating device streams (reference ClUserEvent, a
// "development cancelled" feature there, Worker.cs:487-560): gated streams
// execute hipStreamWaitValue32 on a pinned host word; trigger() stores the
// awaited value.  Words come from a never-freed pinned slab, so a stream can
// never poll released memory.
class UserEvent {
 public:
  UserEvent();
  ~UserEvent();
  uint32_t arm();       // value the next gates wait for
  void trigger();
  bool armed() const { return armed_; }
  const uint32_t* word() const { return word_; }

 private:
  uint32_t* word_ = nullptr;
  uint32_t gen_ = 0;
  bool armed_ = false;
};

// Host rendezvous of the local devices inside one compute() (reference
// phase separation: every device finishes reading and computing before any
// device writes back, Cores.cs:751-831).
class PhaseBarrier {
 public:
  explicit PhaseBarrier(int n) : n_(n) {}
  void arrive_and_wait() {
    std::unique_lock<std::mutex> lk(mu_);
    const int gen = gen_;
    if (++count_ == n_) {
      count_ = 0;
      ++gen_;
      cv_.notify_all();
    } else {
      cv_.wait(lk, [&] { return gen_ != gen || broken_; });
    }
  }
  void arrive_and_drop() {  // a failing device must not block the others
    std::lock_guard<std::mutex> lk(mu_);
    --n_;
    if (count_ >= n_ && count_ > 0) {
      count_ = 0;
      ++gen_;
      cv_.notify_all();
    }
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  int n_, count_ = 0, gen_ = 0;
  bool broken_ = false;
};

// A compute() in which one or more local devices raised.
struct DeviceFailure : std::exception {
  std::vector<int> devices;
  std::string msg;
  void add(int w, const std::string& m) {
    devices.push_back(w);
    msg += (msg.empty() ? "" : "; ") + ("device " + std::to_string(w) + ": " + m);
  }
  const char* what() const noexcept override { return msg.c_str(); }
};

class Cores {
 public:
  Cores(const std::vector<DeviceInfo>& devices, const std::string& source, const CoresConfig& cfg);
  ~Cores();

  int error_code() const { return error_code_; }
  const std::string& error_message() const { return error_; }
  double build_ms() const { return build_ms_; }

  void compute(const ComputeCall& call);

  // ---- modes and knobs ----
  bool enqueue_mode() const { return enqueue_mode_; }
  void set_enqueue_mode(bool on);
  bool async_enqueue = false;
  bool no_compute = false;
  bool fine_grained = false;
  // with fine_grained: this compute's marker is deferred (Worker::defer_marker)
  // until flush_markers(); the device pool sets it per task
  bool defer_marker = false;
  bool smooth = true;
  bool serial = false;  // run devices one after another (isolated timings)
  // Repeat loops with at least this many launches per device are captured
  // into a hipGraph and replayed (0 disables graphs).
  int graph_min_launches = 8;
  // Opt-in overhead-aware balancing (balancer.h predict_split): fits
  // t = a + b·range per device and may leave a device out; single-process
  // jobs only (the law stays the default and the distributed rule).
  bool balancer_predictor = false;
  void set_time_scale(int device, double scale);  // injected heterogeneity (tests/bench)
  // injected fixed cost per compute on a device (ms of host time spent before
  // its work, counted in its measured time): tests of the overhead-aware split
  void set_time_offset(int device, double ms);
  // ---- device-time spans, downloads, host-memory release ----
  bool device_spans = true;  // CEK_DEVICE_SPANS=0: host wall clock instead
  bool single_device_spans = false;  // spans with one device in the job too (CEK_SINGLE_DEVICE_SPANS=1)
  // async enqueue computes' downloads after the next compute's uploads
  // (CEK_DEFER_DOWNLOADS=0: in each compute's own order)
  bool deferred_downloads = true;
  // a system-scope release marker after kernels that may store into
  // zero-copy host memory (per compute in sync mode, once per batch when
  // enqueue mode is left); CEK_ZC_RELEASE=0 turns it off
  bool zc_release = true;
  // ---- failure handling ----
  // When a device fails during compute(): disable it and re-run the call on
  // the remaining devices (single-process jobs only).
  bool auto_failover = false;
  // ---- recording ----
  // schedule recording (sched_log.h)
  using SchedOp = cek::SchedOp;
  bool record_schedule = false;
  // With record_timeline on, the kernels of every compute are bracketed by
  // timing hipEvents on the stream they run on (host clock on the CPU
  // device).  timeline() waits for the recorded work and returns
  // (device, compute id, begin ms, end ms) per span, relative to the first
  // span of that device, then clears the list.
  using TimelineSpan = cek::TimelineSpan;
  bool record_timeline = false;
  // ---- distributed ----
  bool dist_gather_writes = false;
  bool dist_broadcast_reads = false;
  // identical host copies on every rank: each uploads 1/N, RCCL all-gathers
  bool dist_split_reads = false;
  // ---- xGMI fan-out of full `read` arrays ----
  // The reference uploads every `read` array to every device
  // (Worker.cs:833-860): D PCIe copies contending for the host.  With two or
  // more local GPUs computing, an array of at least peer_read_min_bytes that
  // the kernels do not write is instead uploaded 1/D per GPU (each over its
  // own PCIe link) and every GPU pulls the other D-1 chunks straight from its
  // peers' replicas with hipMemcpyPeerAsync: an all-gather over the
  // point-to-point xGMI mesh, one link per peer pair, ordered by events (no
  // host sync).  PCIe carries the array once instead of D times.
  bool peer_reads = true;
  uint64_t peer_read_min_bytes = 1u << 20;
  // ---- pipelines ----
  // event pipeline: issue each blob's D2H on its compute stream
  bool pipeline_writes_on_compute_stream = false;
  // event pipeline: every blob's D2H on one write stream (blob order)
  bool pipeline_writes_one_stream = false;
  // event pipeline: issue every blob's uploads on the main stream, after the
  // full reads (one in-order chain; the copies share the SDMA engine
  // anyway).  With separate read streams, the first call after any
  // device-wide sync left the uploads idle ~5 ms after the full reads and
  // some processes stayed at 14 ms per streamed GEMM call instead of 8
  // (profiles/hostres_streaming.md, tools/hostres_stall_probe.py)
  bool pipeline_reads_on_main_stream = true;
  // explicit blobs: partial arrays alternate over two upload streams (slower:
  // 12.7 vs 7.1 ms for the shells, the extra stream shares a hardware queue)
  bool pipeline_reads_two_streams = false;
  // driver pipeline (Cores.cs:1368-1858): blob k's upload and kernels stay on
  // queue k mod Q, its download goes to one download stream gated by the
  // blob's kernel event, so no blob's D2H waits in a compute queue ahead of a
  // later blob's upload.  Off: the reference's
  // read→compute→write on the one queue.
  bool driver_downloads_own_stream = true;
  // driver pipeline: blob uploads on the main stream (one in-order chain of
  // copies, as the event pipeline's), each blob's queue waiting for its own
  bool driver_reads_on_main_stream = true;
  // ---- host threads and waits ----
  // a mixed CPU + GPU call runs the participant with the largest share on
  // the calling thread (off, the default: the CPU device).  Measured on the
  // wave frame: the GPU inline left the CPU a 1 % share and 0.044 ms per
  // frame, the CPU inline an 11 % share and 0.033 ms (GPU alone 0.030)
  bool inline_largest_share = false;
  // CPU + GPU sets: GPU workers sleep-wait in calls whose previous GPU time
  // for the compute id exceeded sleep_wait_min_ms (CEK_ADAPTIVE_SLEEP=0: off)
  bool adaptive_sleep_waits = true;
  double sleep_wait_min_ms = 0.25;
  // GPU workers wait for their streams by sleeping on a blocking-sync event
  // (off by default; CEK_SLEEP_WAITS=1)
  bool sleep_waits = false;
  // ---- per-worker switches ----
  void set_dynamic_lds(unsigned bytes);
  // device-side enqueue (cek_enqueue): child levels per parent launch, and
  // the errors counted on the devices so far (syncs)
  void set_device_enqueue_levels(int levels);
  int device_enqueue_errors();
  // debug checks: guard tails on new buffers, synchronous checked launches
  void set_debug_checks(bool on);
  bool debug_checks() const { return debug_checks_; }
  // downloads of pinned / registered host memory by a copy kernel instead
  // of hipMemcpyAsync (Worker::kernel_d2h; env CEK_KERNEL_D2H)
  void set_kernel_d2h(bool on) {
    for (auto& w : workers_) w->kernel_d2h = on;
  }
  bool kernel_d2h() const { return !workers_.empty() && workers_[0]->kernel_d2h.load(); }
  uint64_t kernel_d2h_bytes() const {
    uint64_t b = 0;
    for (auto& w : workers_) b += w->kernel_d2h_bytes();
    return b;
  }
  // kernel profiling timestamps (Worker::kernel_times_on)
  void set_kernel_times(bool on) {
    for (auto& w : workers_) w->kernel_times_on = on;
  }
  bool kernel_times_on() const { return !workers_.empty() && workers_[0]->kernel_times_on.load(); }
  std::vector<std::pair<std::string, double>> kernel_times(int dev) { return workers_.at(dev)->kernel_times(); }
  // CUs reserved per GPU for copy kernels (Worker::set_cu_reserve); drains
  // and re-creates the streams
  void set_copy_cus(int n) {
    std::lock_guard<std::recursive_mutex> g(call_mu_);
    if (capturing_) throw Error("copy CUs cannot change during a graph capture");
    for (auto& w : workers_) w->set_cu_reserve(n);
  }
  int copy_cus() const { return workers_.empty() ? 0 : workers_[0]->cu_reserve(); }

  // ---- queries ----
  std::vector<KernelSig> kernels() const;
  int num_devices() const { return static_cast<int>(workers_.size()); }
  int num_global_devices() const { return global_devices_; }
  int global_base() const { return global_base_; }
  const DeviceInfo& device(int i) const { return workers_.at(i)->dev(); }
  uint64_t device_bytes(int i) const { return workers_.at(i)->bytes_allocated(); }
  // identity of device w's host thread pool (0 for a GPU): equal across
  // crunchers that share one (CpuPool::shared)
  uintptr_t cpu_pool_id(int w) const {
    return (w < 0 || w >= static_cast<int>(workers_.size())) ? 0 : workers_[w]->cpu_pool_id();
  }
  // ---- balancer state ----
  bool has_state(int id) const { return state_.count(id) > 0; }
  std::vector<long long> ranges(int id) const;
  std::vector<long long> references(int id) const;
  std::vector<double> benchmarks(int id) const;
  std::vector<std::vector<double>> history(int id) const;
  void set_state(int id, const std::vector<long long>& ranges,
                 const std::vector<std::vector<double>>& history, const std::vector<double>& bench);
  std::vector<int> compute_ids() const;
  int last_compute_id() const { return last_id_; }
  ComputeRecord last_record() const { return last_record_; }
  const FitState* fit_state(int id) const {
    auto it = state_.find(id);
    return it == state_.end() ? nullptr : &it->second.fit;
  }
  // ---- failures ----
  // A disabled device gets no range; the balancer runs over the others.
  void set_device_enabled(int device, bool on);
  bool device_enabled(int device) const { return enabled_.at(device); }
  // Make the next `count` computes on local device `device` fail (tests).
  void inject_failure(int device, int count);
  int failovers() const { return failovers_; }
  // ---- recordings ----
  std::vector<SchedOp> schedule() { return sched_.ops(); }
  void clear_schedule() { sched_.clear(); }
  std::vector<TimelineSpan> timeline();
  // ---- markers ----
  long long markers_reached();
  long long markers_issued();
  std::pair<int, uint64_t> last_marker(int dev) const { return workers_.at(dev)->last_marker(); }
  uint64_t marker_word(int dev, int slot) { return workers_.at(dev)->marker_word(slot); }
  void flush_markers(int dev) { workers_.at(dev)->flush_markers(); }
  // ---- peer topology ----
  // Distinct GPU ordinals of this Cores' devices and hipDeviceCanAccessPeer
  // among them; access is enabled at construction when they span >= 2 GPUs.
  const std::vector<int>& peer_ordinals() const { return peer_.ordinals(); }
  const std::vector<std::vector<int>>& peer_matrix() const { return peer_.matrix(); }
  const std::string& p2p_path() const { return peer_.path(); }
  bool can_peer(int w1, int w2) const { return peer_.can_peer(w1, w2); }

  // ---- operations ----
  void finish();  // synchronise every stream of every device
  void release_array(uint64_t uid);
  // Gate every stream of local device `device` (-1: all) on `ev`: work
  // enqueued afterwards starts only once ev.trigger() (ClUserEvent.cs:102-117).
  void gate(class UserEvent& ev, int device);
  // Raw device pointer of a cached replica (allocates if needed).
  uint64_t device_pointer(int i, const ArraySpec& a);
  void upload(int i, const ArraySpec& a);    // whole array H2D (sync)
  void download(int i, const ArraySpec& a);  // whole array D2H (sync)
  // Keep-resident all-gather inside one process: every device's slice of
  // `a` (by the ranges of compute id `id`) is copied into every other
  // device's replica, GPU↔GPU as peer copies over xGMI (no host bounce).
  // Event-ordered (no host sync in enqueue mode); later computes and
  // downloads wait for the copies on the device.
  void share_slices(int id, const ArraySpec& a, long long local_range);
  void copy_between(int src_dev, const ArraySpec& src, int dst_dev, const ArraySpec& dst,
                    uint64_t bytes);  // device→device (peer/xGMI) copy, sync
  // ---- compute graphs (hipGraph capture of a sequence of computes, graphs.h) ----
  void capture_begin();
  int capture_end();
  void graph_launch(int id, int times, bool sync);
  void graph_destroy(int id);
  bool capturing() const { return capturing_; }
  // Host-resident GEMM C = A·Bᵀ streamed in square shells of P row panels
  // (csrc/shell_gemm.cpp): uploads, kernels and downloads of consecutive
  // shells overlap; C comes back shell by shell.  Synchronous.
  void gemm_host_shells(int local_dev, const std::string& kernel, const ArraySpec& A, const ArraySpec& B,
                        const ArraySpec& C, int M, int N, int K, int panels, int group_m, int BM, int BN, int L);
  void set_distributed(std::shared_ptr<Exchanger> ex, std::shared_ptr<Comm> comm,
                       int global_devices, int global_base);

 private:
  // ---- compute(): cores.cpp ----
  void compute_once(const ComputeCall& call, struct DeviceFailure* failed);
  void balance(struct BalancerState& st, bool first, long long G, long long step);
  void restore_capture_state();  // the modes capture_begin saved (graphs_.saved())
  // ---- the execution shapes: cores_run.cpp ----
  struct Ordering;  // issues and logs what the three run_* shapes enqueue
  bool collective(const ComputeCall& c) const;
  void run_device(int w, const ComputeCall& c, long long ref, long long range, bool pipelined,
                  double* out_ms, uint64_t* h2d, uint64_t* d2h);
  void run_device_body(int w, const ComputeCall& c, long long ref, long long range, bool pipelined,
                  double* out_ms, uint64_t* h2d, uint64_t* d2h);
  void run_3phase(Worker& wk, int gidx, const ComputeCall& c, long long ref, long long range,
                  uint64_t* h2d, uint64_t* d2h);
  void run_event_pipeline(Worker& wk, int gidx, const ComputeCall& c, long long ref,
                          long long range, uint64_t* h2d, uint64_t* d2h);
  void run_driver_pipeline(Worker& wk, int gidx, const ComputeCall& c, long long ref,
                           long long range, uint64_t* h2d, uint64_t* d2h);
  void launch_kernels(Worker& wk, hipStream_t s, const ComputeCall& c, long long ref,
                      long long range);
  void launch_kernels_body(Worker& wk, hipStream_t s, const ComputeCall& c, long long ref,
                           long long range);
  void full_reads(Worker& wk, hipStream_t s, const ComputeCall& c, uint64_t* h2d);
  bool defer_downloads(const Worker& wk) const;
  // issues wk's deferred downloads (downloads_) and the span ends that
  // follow them (spans_); `next` and `c` as in DeferredDownloads::flush
  void flush_downloads(Worker& wk, hipStream_t next = nullptr, const ComputeCall* c = nullptr);
  // the scheduler's modes as the parts take them
  SpanModes span_modes() const {
    return {device_spans, single_device_spans, all_gpu_, global_devices_, enqueue_mode_, async_enqueue};
  }
  PeerView peer_view() const { return {enabled_, global_base_, enqueue_mode_}; }

  PhaseBarrier* phase_ = nullptr;  // set while a hazardous compute runs
  // one compute()/state access at a time per Cores (Python releases the GIL
  // during compute, so two threads may call into the same cruncher)
  mutable std::recursive_mutex call_mu_;
  std::map<int, BalancerState> state_;
  std::vector<double> time_scale_;
  std::vector<double> time_offset_;
  std::vector<bool> enabled_;
  std::vector<int> inject_;
  int failovers_ = 0;
  bool debug_checks_ = false;
  std::string error_;
  int error_code_ = 0;
  double build_ms_ = 0;
  bool enqueue_mode_ = false;
  bool capturing_ = false;
  bool all_gpu_ = true;  // every local device is a GPU (device-time spans feed the balancer)
  bool sleep_this_call_ = false;  // compute_once: GPU waits of this call sleep
  double enqueue_t0_ = 0;
  int last_id_ = 0;
  ComputeRecord last_record_;
  CoresConfig cfg_;
  std::shared_ptr<Exchanger> ex_;
  std::shared_ptr<Comm> comm_;
  int global_devices_ = 0;
  int global_base_ = 0;

  // The workers, then the parts that work through them: destroyed in reverse
  // order, so every part frees its events, graphs and buffers (each with its
  // device current) while the workers and their streams still exist.
  Workers workers_;
  SchedLog sched_{record_schedule};
  Spans spans_{workers_};
  PeerTraffic peer_{workers_, sched_};
  DeferredDownloads downloads_{workers_};
  ComputeGraphs graphs_{workers_};
  std::deque<ShellDims> shell_dims_;  // gemm_host_shells: per local device
};

}  // namespace cek

