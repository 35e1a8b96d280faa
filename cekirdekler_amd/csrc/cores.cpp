#include "cores.h"

#include <cstring>

#include <algorithm>
#include <map>
#include <numeric>
#include <sstream>
#include <thread>

#include "memory.h"
#include "trace.h"
#include "xgmi.h"

namespace cek {

Cores::Cores(const std::vector<DeviceInfo>& devices, const std::string& source,
             const CoresConfig& cfg)
    : cfg_(cfg) {
  smooth = cfg.smooth;
  double t0 = now_ms();
  // One code object per architecture, one module per device.
  std::ostringstream errs;
  int cpu_slot = 0;
  for (size_t i = 0; i < devices.size(); ++i) {
    const auto& d = devices[i];
    std::shared_ptr<Program> prog;
    try {
      prog = Program::build(d, source, cfg.options, d.type == kGPU ? cfg.prebuilt : std::vector<std::string>{});
    } catch (const std::exception& e) {
      errs << "device " << i << " (" << d.name << "): " << e.what() << "\n";
      error_code_ = 1;
      continue;
    }
    if (!prog->ok()) {
      errs << "device " << i << " (" << d.name << ") build failed:\n" << prog->log() << "\n";
      error_code_ = 1;
      continue;
    }
    workers_.emplace_back(new Worker(d, prog, static_cast<int>(workers_.size()), cfg.queue_concurrency,
                                     cfg.no_pipelining, d.type == kGPU ? 0 : cpu_slot++));
  }
  error_ = errs.str();
  if (workers_.empty() && error_code_ == 0) {
    error_code_ = 1;
    error_ = "no device selected";
  }
  global_devices_ = static_cast<int>(workers_.size());
  // the parts size their per-device state now that the workers exist
  spans_.bind();
  downloads_.bind();
  if (const char* e = std::getenv("CEK_DEVICE_SPANS")) device_spans = std::string(e) != "0";
  if (const char* e = std::getenv("CEK_SINGLE_DEVICE_SPANS")) single_device_spans = std::string(e) == "1";
  if (const char* e = std::getenv("CEK_DEFER_DOWNLOADS")) deferred_downloads = std::string(e) != "0";
  if (const char* e = std::getenv("CEK_INLINE_LARGEST")) inline_largest_share = std::string(e) != "0";
  if (const char* e = std::getenv("CEK_ADAPTIVE_SLEEP")) adaptive_sleep_waits = std::string(e) != "0";
  if (const char* e = std::getenv("CEK_KERNEL_D2H")) set_kernel_d2h(std::string(e) != "0");
  if (const char* e = std::getenv("CEK_ZC_RELEASE")) zc_release = std::string(e) != "0";
  // CEK_SLEEP_WAITS=1: GPU workers wait for their streams by sleeping on a
  // blocking-sync event instead of HIP's default wait, leaving the core to a
  // co-executing CPU device.  Off by default: measured on the wave example
  // it adds ~5 µs of wake-up per GPU frame (0.038 -> 0.043 ms) and gains
  // nothing on host-resident co-execution (profiles/round4_session6.md)
  if (const char* e = std::getenv("CEK_SLEEP_WAITS")) sleep_waits = std::string(e) != "0";
  time_scale_.assign(workers_.size(), 1.0);
  time_offset_.assign(workers_.size(), 0.0);
  enabled_.assign(workers_.size(), true);
  inject_.assign(workers_.size(), 0);
  peer_.bind();
  all_gpu_ = std::all_of(workers_.begin(), workers_.end(), [](const std::unique_ptr<Worker>& w) { return w->gpu(); });
  build_ms_ = now_ms() - t0;
}

// Drain, end an open capture, then let the members go in reverse order of
// their declaration (cores.h): the parts free what they own, each with its
// device current, before the workers and their streams are destroyed.
Cores::~Cores() {
  try {
    finish();
  } catch (...) {
  }
  if (capturing_) graphs_.discard_capture(workers_.size());
}

std::vector<KernelSig> Cores::kernels() const {
  if (workers_.empty()) return {};
  return workers_[0]->program().kernels();
}

void Cores::set_time_scale(int device, double scale) {
  if (device < 0 || device >= static_cast<int>(time_scale_.size())) throw Error("bad device index");
  time_scale_[device] = scale;
}

void Cores::set_time_offset(int device, double ms) {
  if (device < 0 || device >= static_cast<int>(time_offset_.size())) throw Error("bad device index");
  time_offset_[device] = ms;
}

void Cores::set_device_enabled(int device, bool on) {
  if (device < 0 || device >= static_cast<int>(enabled_.size())) throw Error("bad device index");
  if (!on && ex_) throw Error("devices cannot be disabled in a distributed job");
  const bool rejoin = on && !enabled_[device];
  enabled_[device] = on;
  // A re-enabled device has no range and no timing: restart every compute id
  // from the equal split so that it rejoins with a real share instead of
  // whatever a stale bench value would give it.
  if (rejoin)
    for (auto& kv : state_) {
      std::fill(kv.second.ranges.begin(), kv.second.ranges.end(), 0LL);
      std::fill(kv.second.bench.begin(), kv.second.bench.end(), 0.0);
      for (auto& h : kv.second.history) std::fill(h.begin(), h.end(), 0.0);
    }
}

void Cores::inject_failure(int device, int count) {
  if (device < 0 || device >= static_cast<int>(inject_.size())) throw Error("bad device index");
  inject_[device] = count;
}

// Runs the reference law over the enabled devices only (all of them unless
// some were disabled); disabled devices keep a zero range.
void Cores::balance(BalancerState& st, bool first, long long G, long long step) {
  const int D = global_devices_;
  std::vector<int> on;
  for (int i = 0; i < D; ++i)
    if (i < global_base_ || i >= global_base_ + num_devices() || enabled_[i - global_base_]) on.push_back(i);
  if (on.empty()) throw Error("every device is disabled");
  if (static_cast<int>(on.size()) == D) {
    if (first)
      initial_split(D, smooth, st.history, G, st.ranges, step);
    else if (!(balancer_predictor && !ex_ && predict_split(st.fit, st.bench, st.last_wall_ms, G, st.ranges, step, st.calls >= 2)))
      load_balance(st.bench, smooth, st.history, G, st.ranges, step);
    return;
  }
  const size_t n = on.size();
  std::vector<long long> r(n);
  std::vector<double> b(n);
  std::vector<std::vector<double>> h(st.history.size(), std::vector<double>(n));
  for (size_t j = 0; j < n; ++j) {
    r[j] = st.ranges.empty() ? 0 : st.ranges[on[j]];
    b[j] = st.bench.empty() ? 0.0 : st.bench[on[j]];
    for (size_t d = 0; d < st.history.size(); ++d) h[d][j] = st.history[d][on[j]];
  }
  const bool sub_first = first || std::all_of(r.begin(), r.end(), [](long long x) { return x == 0; });
  if (sub_first)
    initial_split(static_cast<int>(n), smooth, h, G, r, step);
  else
    load_balance(b, smooth, h, G, r, step);
  st.ranges.assign(D, 0);
  for (size_t j = 0; j < n; ++j) {
    st.ranges[on[j]] = r[j];
    for (size_t d = 0; d < st.history.size(); ++d) st.history[d][on[j]] = h[d][j];
  }
}

void Cores::set_device_enqueue_levels(int levels) {
  if (levels < 0 || levels > kDynLevels - 1)
    throw Error("device enqueue levels must be in [0, " + std::to_string(kDynLevels - 1) + "]");
  for (auto& w : workers_) w->device_enqueue_levels = levels;
}

void Cores::set_debug_checks(bool on) {
  debug_checks_ = on;
  for (auto& w : workers_) w->debug_checks = on;
}

int Cores::device_enqueue_errors() {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  int e = 0;
  for (auto& w : workers_) e += w->device_enqueue_errors();
  return e;
}

void Cores::set_dynamic_lds(unsigned bytes) {
  for (auto& w : workers_) w->set_dynamic_lds(bytes);
}

void Cores::set_distributed(std::shared_ptr<Exchanger> ex, std::shared_ptr<Comm> comm,
                            int global_devices, int global_base) {
  ex_ = std::move(ex);
  comm_ = std::move(comm);
  global_devices_ = global_devices;
  global_base_ = global_base;
  state_.clear();
}

void Cores::set_enqueue_mode(bool on) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  if (capturing_) throw Error("enqueue mode cannot change during a graph capture");
  if (on && !enqueue_mode_) {
    enqueue_t0_ = now_ms();
  } else if (!on && enqueue_mode_) {
    spans_.close_batch();
    if (zc_release)  // one system-scope release per device for the whole batch (zero-copy stores)
      for (auto& w : workers_)
        if (w->gpu()) {
          w->join_streams(w->main_stream());
          w->system_release(w->main_stream());
        }
    finish();
    double el = now_ms() - enqueue_t0_;
    auto it = state_.find(last_id_);
    std::vector<double> ms(num_devices());
    for (int w = 0; w < num_devices(); ++w) {
      // GPU: union of this device's timed spans; CPU device: wall clock
      double dev = workers_[w]->gpu() ? spans_.enqueue_ms(w) : -1.0;
      if (!all_gpu_) dev = -1.0;  // mixed CPU+GPU: one clock for everybody
      ms[w] = (dev > 0 ? dev : el) * time_scale_[w];
    }
    // every rank leaves enqueue mode together: exchange so all ranks keep the
    // identical benchmark vector (and hence derive the identical next split)
    std::vector<double> all = ex_ ? ex_->allgather(ms) : ms;
    if (it != state_.end()) {
      if (ex_ && all.size() == it->second.bench.size()) {
        it->second.bench = all;
      } else {
        for (int w = 0; w < num_devices(); ++w) {
          size_t g = static_cast<size_t>(global_base_ + w);
          if (g < it->second.bench.size()) it->second.bench[g] = ms[w];
        }
      }
    }
  }
  enqueue_mode_ = on;
}

std::vector<long long> Cores::ranges(int id) const {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  auto it = state_.find(id);
  return it == state_.end() ? std::vector<long long>{} : it->second.ranges;
}
std::vector<long long> Cores::references(int id) const {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  auto it = state_.find(id);
  return it == state_.end() ? std::vector<long long>{} : it->second.references;
}
std::vector<double> Cores::benchmarks(int id) const {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  auto it = state_.find(id);
  return it == state_.end() ? std::vector<double>{} : it->second.bench;
}
std::vector<std::vector<double>> Cores::history(int id) const {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  auto it = state_.find(id);
  return it == state_.end() ? std::vector<std::vector<double>>{} : it->second.history;
}
std::vector<int> Cores::compute_ids() const {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  std::vector<int> out;
  for (auto& kv : state_) out.push_back(kv.first);
  return out;
}

void Cores::set_state(int id, const std::vector<long long>& ranges,
                      const std::vector<std::vector<double>>& history, const std::vector<double>& bench) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  auto& st = state_[id];
  st.ranges = ranges;
  st.history = history;
  st.bench = bench;
  st.global_range = std::accumulate(ranges.begin(), ranges.end(), 0LL);
  st.references.assign(ranges.size(), 0);
  long long acc = st.global_offset;
  for (size_t i = 0; i < ranges.size(); ++i) {
    st.references[i] = acc;
    acc += ranges[i];
  }
}

long long Cores::markers_reached() {
  long long r = 0;
  for (auto& w : workers_) r += w->markers_reached();
  return r;
}

long long Cores::markers_issued() {
  long long r = 0;
  for (auto& w : workers_) r += w->markers_issued();
  return r;
}

void Cores::capture_begin() {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  if (capturing_) throw Error("capture_begin: already capturing");
  for (auto& w : workers_)
    if (!w->gpu()) throw Error("compute graphs need GPU devices only (the CPU device runs computes at once)");
  if (debug_checks_) throw Error("compute graphs cannot be captured with debug checks on (they synchronise)");
  for (auto& w : workers_) {
    w->wait();
    flush_downloads(*w);
    w->sync_all();
  }
  const CaptureSaved saved = {device_spans, peer_reads, async_enqueue, fine_grained, enqueue_mode_, record_timeline,
                              graph_min_launches, kernel_times_on()};
  set_kernel_times(false);  // stamped launches are not captured (their events would never be recorded)
  device_spans = false;
  record_timeline = false;
  peer_reads = false;
  async_enqueue = false;
  fine_grained = false;
  graph_min_launches = 0;
  enqueue_mode_ = true;  // split frozen, no syncs (state is restored by capture_end)
  try {
    graphs_.begin(saved);
  } catch (...) {
    restore_capture_state();
    throw;
  }
  capturing_ = true;
}

void Cores::restore_capture_state() {
  const CaptureSaved& saved = graphs_.saved();
  device_spans = saved.device_spans;
  peer_reads = saved.peer_reads;
  async_enqueue = saved.async_enqueue;
  fine_grained = saved.fine_grained;
  graph_min_launches = saved.graph_min_launches;
  enqueue_mode_ = saved.enqueue_mode;
  record_timeline = saved.record_timeline;
  set_kernel_times(saved.kernel_times);
}

int Cores::capture_end() {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  if (!capturing_) throw Error("capture_end: not capturing");
  std::string err;
  const int id = graphs_.end(err);
  capturing_ = false;
  restore_capture_state();
  spans_.forget();
  if (!err.empty()) throw Error(err);
  return id;
}

void Cores::graph_launch(int id, int times, bool sync) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  graphs_.launch(id, times, sync);
}

void Cores::graph_destroy(int id) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  graphs_.destroy(id);
}

void Cores::finish() {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  if (capturing_) throw Error("finish() during a graph capture (end the capture first)");
  for (auto& w : workers_) {
    w->wait();
    flush_downloads(*w);
    w->sync_all();
  }
  peer_.gather_pending = false;  // every gather copy (on the main streams) is done
}

// A deferred download of the array being released still targets its host
// buffer: issue it and let it land before the device buffer goes away (the
// host buffer is alive for the duration of the caller's __del__).
void Cores::release_array(uint64_t uid) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  for (size_t w = 0; w < workers_.size(); ++w) {
    Worker& wk = *workers_[w];
    const std::vector<hipStream_t> streams = downloads_.streams_holding(static_cast<int>(w), uid);
    if (!streams.empty()) {
      flush_downloads(wk);
      if (wk.gpu())
        for (hipStream_t st : streams) CEK_HIP(hipStreamSynchronize(st));
    }
    wk.release(uid);
  }
}

uint64_t Cores::device_pointer(int i, const ArraySpec& a) {
  Worker& w = *workers_.at(i);
  w.set_device();
  return reinterpret_cast<uint64_t>(w.buffer(a));
}

void Cores::upload(int i, const ArraySpec& a) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  Worker& w = *workers_.at(i);
  w.set_device();
  flush_downloads(w);
  hipStream_t s = w.main_stream();
  peer_.wait_gather(w, s);
  w.h2d(s, a, 0, a.bytes / a.elem_size);
  if (w.gpu()) CEK_HIP(hipStreamSynchronize(s));
}

void Cores::download(int i, const ArraySpec& a) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  Worker& w = *workers_.at(i);
  w.set_device();
  flush_downloads(w);
  hipStream_t s = w.main_stream();
  peer_.wait_gather(w, s);
  w.d2h(s, a, 0, a.bytes / a.elem_size);
  if (w.gpu()) CEK_HIP(hipStreamSynchronize(s));
}

void Cores::copy_between(int src_dev, const ArraySpec& src, int dst_dev, const ArraySpec& dst,
                         uint64_t bytes) {
  Worker& ws = *workers_.at(src_dev);
  Worker& wd = *workers_.at(dst_dev);
  if (bytes > src.bytes || bytes > dst.bytes) throw Error("copy_between: size exceeds array");
  if (!ws.gpu() && !wd.gpu()) {
    std::memcpy(dst.host, src.host, bytes);
    return;
  }
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  peer_.copy_between(src_dev, src, dst_dev, dst, bytes, enqueue_mode_);
}

void Cores::share_slices(int id, const ArraySpec& a, long long local_range) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  auto it = state_.find(id);
  if (it == state_.end()) throw Error("share_slices: unknown compute id");
  if (capturing_) throw Error("share_slices during a graph capture");
  peer_.share_slices(it->second, a, local_range, peer_view());
}

// ---------------------------------------------------------------- UserEvent --

namespace {
std::mutex g_ue_mu;
uint32_t* g_ue_slab = nullptr;
int g_ue_next = 0;
constexpr int kUserEventSlots = 4096;
}  // namespace

UserEvent::UserEvent() {
  std::lock_guard<std::mutex> g(g_ue_mu);
  if (!g_ue_slab) {
    bool pinned = false;
    g_ue_slab = static_cast<uint32_t*>(host_alloc(kUserEventSlots * sizeof(uint32_t), 4096, &pinned));
    std::memset(g_ue_slab, 0, kUserEventSlots * sizeof(uint32_t));
  }
  if (g_ue_next >= kUserEventSlots) throw Error("too many user events in this process");
  word_ = &g_ue_slab[g_ue_next++];
}

UserEvent::~UserEvent() {
  if (armed_) trigger();  // never leave a stream blocked on a dead event
}

uint32_t UserEvent::arm() {
  armed_ = true;
  return gen_ + 1;
}

void UserEvent::trigger() {
  __atomic_store_n(word_, gen_ + 1, __ATOMIC_RELEASE);
  ++gen_;
  armed_ = false;
}

void Cores::gate(UserEvent& ev, int device) {
  const uint32_t v = ev.arm();
  for (int w = 0; w < num_devices(); ++w)
    if (device < 0 || device == w) workers_[w]->gate_all_streams(ev.word(), v);
}

std::vector<Cores::TimelineSpan> Cores::timeline() {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  return spans_.timeline();
}

// ------------------------------------------------------------- compute --

void Cores::compute(const ComputeCall& c) {
  std::lock_guard<std::recursive_mutex> call_guard(call_mu_);
  DeviceFailure f;
  compute_once(c, (auto_failover && !ex_) ? &f : nullptr);
  if (f.devices.empty()) return;
  // Failover: the surviving devices' slices are complete; each failed
  // device's slice is recomputed on a surviving device (from the same host
  // inputs), and the failed device is dropped from later splits.
  for (int w : f.devices) enabled_[w] = false;
  int survivor = -1;
  for (int w = 0; w < num_devices() && survivor < 0; ++w)
    if (enabled_[w]) survivor = w;
  if (survivor < 0) throw Error(std::string("every device failed: ") + f.what());
  auto& st = state_[c.compute_id];
  // keep-resident arrays: the recomputed slices must reach every surviving
  // replica too (the regular gather was skipped for this call)
  std::vector<int> gather_idx;
  for (size_t i = 0; i < c.arrays.size(); ++i)
    if (c.arrays[i].gather && !c.arrays[i].zc) gather_idx.push_back(static_cast<int>(i));
  const bool regather = !gather_idx.empty() && !comm_ && num_devices() > 1;
  peer_.call_gathers = regather;  // the survivor records its kernels-done event
  for (int w : f.devices) {
    const int g = global_base_ + w;
    double ms = 0;
    uint64_t h = 0, d = 0;
    try {
      run_device(survivor, c, st.references[g], st.ranges[g], false, &ms, &h, &d);
    } catch (...) {
      peer_.call_gathers = false;
      throw;
    }
  }
  peer_.call_gathers = false;
  if (regather) {
    std::vector<std::vector<std::pair<long long, long long>>> owned(num_devices());
    for (int w = 0; w < num_devices(); ++w)
      if (enabled_[w]) owned[w].push_back({st.references[global_base_ + w], st.ranges[global_base_ + w]});
    for (int w : f.devices) owned[survivor].push_back({st.references[global_base_ + w], st.ranges[global_base_ + w]});
    peer_.d2d = D2DCount();
    last_record_.gather_bytes = peer_.issue_gather(c, st, gather_idx, peer_view(), &owned);
  }
  ++failovers_;
}

void Cores::compute_once(const ComputeCall& c, DeviceFailure* failed) {
  if (error_code_ != 0) throw Error("cannot compute, initialisation failed: " + error_);
  const long long G = c.global_range, L = c.local_range;
  if (G <= 0) throw Error("global range must be positive");
  if (L <= 0 || L > 1024) throw Error("local range must be in [1, 1024]");
  if (G % L != 0) throw Error("global range must be a multiple of local range");
  for (auto& k : c.kernels)
    if (!workers_[0]->program().has(k)) throw Error("unknown kernel: " + k);
  if (!c.repeat_kernel.empty() && !workers_[0]->program().has(c.repeat_kernel))
    throw Error("unknown repeat kernel: " + c.repeat_kernel);
  // Every kernel of a compute receives the same array list (Worker.cs:990-1021
  // binds them positionally); a count mismatch would shift the hidden offset
  // argument onto a pointer and make the kernel address wild memory.
  {
    const int nargs = static_cast<int>(c.arrays.size());
    auto check = [&](const std::string& k) {
      const int ar = workers_[0]->program().arity(k);
      if (ar >= 0 && ar != nargs)
        throw Error("kernel " + k + " takes " + std::to_string(ar) + " array parameter(s) but compute passes " +
                    std::to_string(nargs));
    };
    for (auto& k : c.kernels) check(k);
    if (!c.repeat_kernel.empty()) check(c.repeat_kernel);
  }
  const int D = global_devices_;
  const int nloc = num_devices();
  // equal blobs split every device's range, so ranges move in steps of
  // blobs × unit; explicit blob bounds describe the whole range of the one
  // holding device and put no constraint on the step (their count need not
  // divide the range: 16 square shells plus split ones)
  const long long B = c.blob_bounds.empty() ? std::max(1, c.blobs) : 1;
  const bool pipe_req = c.pipeline && !cfg_.no_pipelining;
  const long long U = c.granularity > 0 ? c.granularity : L;  // balancer unit
  if (U % L != 0) throw Error("granularity must be a multiple of the local range");
  if (G % U != 0) throw Error("global range must be a multiple of the granularity");
  TraceRange tr(trace_enabled() ? "cek.compute.id" + std::to_string(c.compute_id) : std::string());
  double wall0 = now_ms();

  auto it = state_.find(c.compute_id);
  bool fresh = it == state_.end() || it->second.global_range != G ||
               (it->second.local_range != 0 && it->second.local_range != L) ||
               static_cast<int>(it->second.ranges.size()) != D;
  BalancerState& st = state_[c.compute_id];
  if (fresh) {
    st = BalancerState();
    st.history.assign(kHistoryDepth, std::vector<double>(D, 0.0));
    st.bench.assign(D, 0.0);
    st.global_range = G;
    st.local_range = L;
  }
  st.global_offset = c.global_offset;
  st.local_range = L;  // (restored states carry no local range)
  if (st.history.size() != static_cast<size_t>(kHistoryDepth))
    st.history.assign(kHistoryDepth, std::vector<double>(D, 0.0));
  if (st.bench.size() != static_cast<size_t>(D)) st.bench.assign(D, 0.0);
  const bool first = fresh || std::all_of(st.ranges.begin(), st.ranges.end(), [](long long r) { return r == 0; });
  if (!(enqueue_mode_ && !first)) {
    int active = 0;
    for (int i = 0; i < D; ++i)
      if (i < global_base_ || i >= global_base_ + nloc || enabled_[i - global_base_]) ++active;
    if (first) {
      // Cores.cs:569-596
      std::vector<long long> eq(active, G / std::max(active, 1));
      if (active) eq[0] += G - (G / active) * active;
      bool b1 = std::all_of(eq.begin(), eq.end(), [&](long long r) { return r >= B * U; });
      long long step = (b1 && pipe_req && G >= B * U) ? B * U : U;
      balance(st, true, G, step);
    } else {
      bool b1 = true;
      for (int i = 0; i < D; ++i)
        if (st.ranges[i] != 0 && st.ranges[i] < B * U) b1 = false;
      long long step = (b1 && pipe_req && G >= B * U) ? B * U : U;
      balance(st, false, G, step);
    }
  }
  st.references.assign(D, 0);
  long long acc = c.global_offset;
  for (int i = 0; i < D; ++i) {
    st.references[i] = acc;
    acc += st.ranges[i];
  }
  // Host-memory hazard: an array read whole by every device and written back
  // by slices.  With several local devices the phases must be separated.
  bool hazard = false;
  if (nloc > 1)
    for (auto& a : c.arrays)
      if (!a.zc && a.read && !a.partial && a.write) hazard = true;
  // Pipelining eligibility (Cores.cs:624-652), decided per call for all devices.
  // keep-resident gather arrays (in process; across ranks RCCL does it)
  std::vector<int> gather_idx;
  for (size_t i = 0; i < c.arrays.size(); ++i)
    if (c.arrays[i].gather && !c.arrays[i].zc) gather_idx.push_back(static_cast<int>(i));
  if (!gather_idx.empty() && capturing_) throw Error("keep-resident gather arrays cannot be captured into a graph");
  if (!gather_idx.empty() && ex_ && !comm_ && global_devices_ > nloc)
    throw Error("gather across ranks needs an RCCL communicator (DistributedCruncher(comm=True))");
  peer_.call_gathers = !gather_idx.empty() && !comm_ && nloc > 1;
  bool pipelined = pipe_req && c.repeats <= 1 && !enqueue_mode_ && !hazard && gather_idx.empty();
  if (!c.blob_bounds.empty()) {
    // explicit blobs describe the whole range on one device
    const auto& bb = c.blob_bounds;
    bool ok = bb.size() >= 2 && bb.front() == 0 && bb.back() == G && c.pipeline_event;
    for (size_t k = 1; ok && k < bb.size(); ++k) ok = bb[k] > bb[k - 1] && bb[k] % L == 0;
    if (!ok) throw Error("blob_bounds must rise from 0 to the global range in whole work-groups (event pipeline)");
    for (const auto& a : c.arrays)
      if (!a.blob_begin.empty() && (a.blob_begin.size() != bb.size() - 1 || a.blob_count.size() != bb.size() - 1))
        throw Error("an array's blob slices must have one entry per blob");
    int holders = 0;
    for (int i = 0; i < D; ++i) holders += st.ranges[i] > 0;
    if (holders != 1) pipelined = false;  // split over devices: the plain path
  } else {
    for (int i = 0; i < D && pipelined; ++i)
      if (st.ranges[i] != 0 && (st.ranges[i] % (B * U) != 0 || st.ranges[i] < B * U)) pipelined = false;
  }
  if (collective(c)) pipelined = false;

  // A GPU that shares the call with a CPU device sleeps on its stream when
  // its last time for this compute id was long: a spinning wait would take
  // a core (an SMT sibling) from the CPU device's threads for milliseconds.
  // Short GPU waits (a 0.03 ms wave frame) keep spinning, where a wake-up
  // would cost more than the core.
  sleep_this_call_ = false;
  if (!all_gpu_ && adaptive_sleep_waits)
    for (int w = 0; w < nloc; ++w)
      if (workers_[w]->gpu() && st.bench[global_base_ + w] > sleep_wait_min_ms) sleep_this_call_ = true;
  std::vector<double> ms(nloc, 0.0);
  std::vector<uint64_t> h2d(nloc, 0), d2h(nloc, 0);
  // xGMI fan-out of full reads, enqueued before the per-device work (its
  // time lands on the devices' streams, inside their measured span only
  // through the event waits in full_reads)
  peer_.d2d = D2DCount();
  if (peer_.gather_pending)  // the last gather's copies finish before this call touches any replica
    for (int w = 0; w < nloc; ++w)
      if (workers_[w]->gpu()) {
        workers_[w]->set_device();
        peer_.wait_gather(*workers_[w], workers_[w]->main_stream());
      }
  peer_.stage_reads(c, st.ranges, h2d, peer_view(),
                    peer_reads && !(comm_ && (dist_broadcast_reads || dist_split_reads)), peer_read_min_bytes);
  DeviceFailure failure;
  int participants = 0;
  std::vector<char> part(nloc, 0);
  for (int w = 0; w < nloc; ++w)
    if (st.ranges[global_base_ + w] > 0 || collective(c)) {
      part[w] = 1;
      ++participants;
    }
  PhaseBarrier phase(participants);
  if (hazard && !enqueue_mode_ && participants > 1) phase_ = &phase;
  struct ResetPhase {
    PhaseBarrier*& p;
    ~ResetPhase() { p = nullptr; }
  } reset_phase{phase_};
  // A device with an empty range does no device work; with at most one
  // participant there is nothing to overlap, so no worker-thread hand-off
  // (a device the overhead-aware balancer left out costs nothing per call).
  if (nloc == 1 || (serial && !phase_) || participants <= 1) {
    for (int w = 0; w < nloc; ++w) {
      int g = global_base_ + w;
      try {
        run_device(w, c, st.references[g], st.ranges[g], pipelined, &ms[w], &h2d[w], &d2h[w]);
      } catch (const std::exception& e) {
        failure.add(w, e.what());
      }
    }
  } else {
    // One participant runs on the calling thread: a hand-off fewer per call
    // (the wave frame's GPU+CPU split pays one wake-up instead of two).  A
    // CPU device is preferred there — its work is the calling thread plus
    // the CPU pool either way, and the GPU workers are posted first so
    // their launches go out while the CPU computes.
    // Option (inline_largest_share): the participant holding the largest
    // share runs here instead (measured slower on the wave frame, off).
    int inline_w = -1;
    if (inline_largest_share && !all_gpu_) {
      for (int w = 0; w < nloc; ++w)
        if (part[w] && (inline_w < 0 || st.ranges[global_base_ + w] > st.ranges[global_base_ + inline_w] ||
                        (st.ranges[global_base_ + w] == st.ranges[global_base_ + inline_w] && !workers_[w]->gpu())))
          inline_w = w;
    } else {
      for (int w = 0; w < nloc; ++w)
        if (part[w] && (inline_w < 0 || !workers_[w]->gpu())) inline_w = w;
    }
    for (int w = 0; w < nloc; ++w) {
      if (!part[w] || w == inline_w) continue;
      int g = global_base_ + w;
      long long ref = st.references[g], rng = st.ranges[g];
      workers_[w]->post([=, &c, &ms, &h2d, &d2h] {
        run_device(w, c, ref, rng, pipelined, &ms[w], &h2d[w], &d2h[w]);
      });
    }
    // the calling thread's current device is the caller's (torch allocates
    // on it): restored after a GPU participant ran here
    struct RestoreDevice {
      int dev = -1;
      explicit RestoreDevice(bool gpu) {
        if (gpu && hipGetDevice(&dev) != hipSuccess) dev = -1;
      }
      ~RestoreDevice() {
        if (dev >= 0) (void)hipSetDevice(dev);
      }
    } restore(inline_w >= 0 && workers_[inline_w]->gpu());
    for (int w = 0; w < nloc; ++w) {
      if (part[w] && w != inline_w) continue;
      try {
        run_device(w, c, st.references[global_base_ + w], part[w] ? st.ranges[global_base_ + w] : 0,
                   pipelined, &ms[w], &h2d[w], &d2h[w]);
      } catch (const std::exception& e) {
        failure.add(w, e.what());
      }
    }
    for (int w = 0; w < nloc; ++w) {
      if (!part[w] || w == inline_w) continue;
      try {
        workers_[w]->wait();
      } catch (const std::exception& e) {
        failure.add(w, e.what());
      }
    }
  }
  if (!failure.devices.empty()) {
    peer_.call_gathers = false;
    if (!failed) throw Error(failure.what());
    *failed = failure;
  }
  uint64_t gathered = 0;
  if (peer_.call_gathers) {
    peer_.call_gathers = false;
    gathered = peer_.issue_gather(c, st, gather_idx, peer_view());
  }
  last_id_ = c.compute_id;
  if (!enqueue_mode_) {
    std::vector<double> all = ms;
    if (ex_) all = ex_->allgather(ms);
    if (static_cast<int>(all.size()) == D) st.bench = all;
  }
  ++st.calls;
  last_record_.compute_id = c.compute_id;
  last_record_.wall_ms = now_ms() - wall0;
  st.last_wall_ms = last_record_.wall_ms;
  last_record_.ranges = st.ranges;
  last_record_.references = st.references;
  last_record_.device_ms = st.bench;
  last_record_.h2d_bytes = std::accumulate(h2d.begin(), h2d.end(), 0ull);
  last_record_.d2h_bytes = std::accumulate(d2h.begin(), d2h.end(), 0ull);
  last_record_.p2p_bytes = peer_.d2d.bytes;
  last_record_.gather_bytes = gathered;
  last_record_.staged_bytes = peer_.d2d.staged;
  last_record_.p2p_path = peer_.d2d.path();
  last_record_.pipelined = pipelined;
}

}  // namespace cek
