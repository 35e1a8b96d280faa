// Native self-test of the C++ runtime on the host CPU device, built with
// AddressSanitizer + UndefinedBehaviorSanitizer (sanitizers on
// the host runtime).  Exercises the balancer law, the JIT front end, and
// Cores::compute on logical CPU devices: plain, event/driver pipelines,
// repeats + sync kernel, phase separation, failover; and the worker's parts
// that need no GPU: lane ids, the job thread, markers and replicas of a CPU
// worker.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <numeric>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "balancer.h"
#include "cores.h"
#include "device.h"
#include "jit.h"
#include "job_thread.h"
#include "lanes.h"
#include "worker.h"

using namespace cek;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static const char* kSrc = R"(
__global__ void inc(float* x) { x[get_global_id(0)] += 1.0f; }
__global__ void saxpy(const float* a, const float* x, float* y) {
  long long i = get_global_id(0); y[i] = a[0] * x[i] + y[i]; }
__global__ void count(float* x, int* c) { if (get_global_id(0) == 0) c[0] += 1; }
__global__ void incc(float* x, int* c) { x[get_global_id(0)] += 1.0f; }
__global__ void groupsum(const float* x, float* out) {
  __shared__ float s[64];
  int l = (int)get_local_id(0);
  s[l] = x[get_global_id(0)];
  __syncthreads();
  for (int w = 32; w > 0; w >>= 1) { if (l < w) s[l] += s[l + w]; __syncthreads(); }
  if (l == 0) out[get_global_id(0) / 64] = s[0];
}
)";

static ArraySpec spec(uint64_t uid, void* p, uint64_t bytes, int esize) {
  ArraySpec a;
  a.uid = uid;
  a.host = p;
  a.bytes = bytes;
  a.elem_size = esize;
  return a;
}

static void test_balancer() {
  for (int trial = 0; trial < 50; ++trial) {
    const int n = 2 + trial % 5;
    const long long step = 64 * (1 + trial % 3), total = step * (40 + trial);
    std::vector<std::vector<double>> hist(kHistoryDepth, std::vector<double>(n, 0.0));
    std::vector<long long> r;
    initial_split(n, true, hist, total, r, step);
    for (int call = 0; call < 20; ++call) {
      std::vector<double> bench(n);
      for (int i = 0; i < n; ++i) bench[i] = static_cast<double>(r[i]) / (1.0 + i) + 0.1;
      load_balance(bench, true, hist, total, r, step);
      CHECK(std::accumulate(r.begin(), r.end(), 0LL) == total);
      for (long long x : r) CHECK(x % step == 0 && x >= 0);
    }
  }
}

static void test_jit() {
  auto ks = parse_kernels(kSrc);
  CHECK(ks.size() == 5);
  for (auto& k : ks) {
    if (k.name == "saxpy") CHECK(k.arity == 3);
    if (k.name == "inc") CHECK(k.arity == 1);
  }
  const std::string g = gpu_rewrite(kSrc);
  CHECK(g.find("__cek_off") != std::string::npos);
  CHECK(is_opencl_dialect("__kernel void k(__global float* a) { a[0] = 1; }"));
}

// byte_chunk against the two splits it replaced: the read fan-out's (4 KiB
// chunks) and the distributed split upload's (whole elements).
static void test_byte_chunk() {
  const uint64_t sizes[] = {0, 1, 4095, 4096, 4097, (1u << 20) + 3};
  const uint64_t aligns[] = {4096, 1, 2, 4, 8};
  for (uint64_t bytes : sizes)
    for (int P : {1, 2, 3, 8})
      for (uint64_t align : aligns)
        for (int k = 0; k < P; ++k) {
          uint64_t chunk = (bytes + P - 1) / P, off, len;
          if (align == 4096) {  // stage_peer_reads
            chunk = (chunk + 4095) / 4096 * 4096;
            off = std::min<uint64_t>(k * chunk, bytes);
            len = std::min<uint64_t>(chunk, bytes - off);
          } else {  // full_reads with dist_split_reads
            const int elem_size = static_cast<int>(align);
            chunk = (chunk + elem_size - 1) / elem_size * elem_size;
            off = std::min<uint64_t>(k * chunk, bytes);
            len = std::min<uint64_t>(chunk, bytes - off);
          }
          const auto got = byte_chunk(bytes, P, align, k);
          CHECK(got.first == off && got.second == len);
        }
}

// The 23 lane ids are distinct and below kNoLane; a CPU device has no stream
// behind any of them, and a stream of nobody's is kNoLane.
static void test_lane_ids() {
  std::set<int> ids = {main_lane_id()};
  for (int q = 0; q < 16; ++q) ids.insert(compute_lane_id(q));
  for (int h = 0; h < 2; ++h)
    for (int r = 0; r < 3; ++r) ids.insert(pipe_lane_id(h, r));
  CHECK(ids.size() == 23);
  const DeviceInfo cpu = cpu_info(2);
  for (int qconc : {1, 3}) {
    LaneTable lanes(cpu, qconc);
    for (int id : ids) {
      CHECK(id >= 0 && id < kNoLane);
      CHECK(lanes.open(id) == nullptr);
      CHECK(lanes.stream(id) == nullptr);
    }
    int created = 0;
    lanes.for_each_created([&](hipStream_t, int) { ++created; });
    CHECK(created == 0);
    int not_a_stream = 0;
    CHECK(lanes.id_of(reinterpret_cast<hipStream_t>(&not_a_stream)) == kNoLane);
  }
}

static void test_job_thread() {
  const double saved = JobThread::spin_us;
  for (double us : {0.0, 50.0}) {
    JobThread::spin_us = us;
    for (bool spin : {false, true}) {
      std::atomic<int> ran{0}, first_calls{0};
      {
        JobThread jt(spin, [&] { ++first_calls; });
        for (int round = 0; round < 3; ++round) {
          for (int i = 0; i < 100; ++i) jt.post([&] { ++ran; });
          jt.wait();
          CHECK(ran == 100 * (round + 1));
        }
        CHECK(first_calls == 1);
        // the first of two exceptions comes out of wait() once
        jt.post([] { throw Error("first"); });
        jt.post([] { throw Error("second"); });
        jt.post([&] { ++ran; });
        std::string what;
        try {
          jt.wait();
        } catch (const Error& e) {
          what = e.what();
        }
        CHECK(what == "first");
        CHECK(ran == 301);
        bool clean = true;
        try {
          jt.wait();
        } catch (...) {
          clean = false;
        }
        CHECK(clean);
        // destruction runs what is still queued: the thread is held in its
        // current job until the destructor has asked it to stop
        std::atomic<bool> go{false};
        jt.post([&] {
          while (!go) std::this_thread::yield();
        });
        for (int i = 0; i < 50; ++i) jt.post([&] { ++ran; });
        std::thread releaser([&] {
          std::this_thread::sleep_for(std::chrono::milliseconds(20));
          go = true;
        });
        jt.stop();
        releaser.join();
        CHECK(ran == 351);
      }
    }
  }
  JobThread::spin_us = saved;
}

// A CPU worker's markers are reached when issued, and its replicas are the
// host arrays themselves.
static void test_cpu_worker_parts() {
  Worker w(cpu_info(2), nullptr, 0, 3, false);
  CHECK(!w.gpu() && w.main_stream() == nullptr && w.compute_lane(2).id == 3 && w.pipe_lane(1, 2).id == 22);
  for (int i = 0; i < 3; ++i) {
    if (i == 0) w.add_marker(nullptr, true);
    if (i == 1) w.defer_marker(nullptr);
    if (i == 2) w.flush_markers();
    CHECK(w.markers_issued() == (i < 2 ? i + 1 : 2));
    CHECK(w.last_marker() == std::make_pair(-1, static_cast<uint64_t>(w.markers_issued())));
    CHECK(w.markers_reached() == w.markers_issued());
    CHECK(!w.has_deferred_markers());
    CHECK(w.marker_word(-1) == static_cast<uint64_t>(w.markers_issued()));
  }

  std::vector<float> x(16), y(16);
  const ArraySpec sx = spec(41, x.data(), 64, 4), sy = spec(42, y.data(), 64, 4);
  CHECK(w.buffer(sx) == x.data());
  std::vector<std::pair<uint64_t, void*>> log;
  w.set_capture_log(&log);
  CHECK(w.buffer(sx) == x.data() && w.buffer(sy) == y.data() && w.buffer(sx) == x.data());
  w.set_capture_log(nullptr);
  CHECK(w.buffer(sy) == y.data());
  const std::vector<std::pair<uint64_t, void*>> want = {{41, x.data()}, {42, y.data()}, {41, x.data()}};
  CHECK(log == want);
  CHECK(!w.buffer_is(41, x.data()));  // a CPU device keeps no replica to compare with
  CHECK(w.bytes_allocated() == 0);
  w.release(41);
  w.release_all();
  CHECK(w.bytes_allocated() == 0);
  std::atomic<int> ran{0};
  w.post([&] { ++ran; });
  w.wait();
  CHECK(ran == 1);
}

static void test_cores() {
  DeviceInfo cpu = cpu_info(2);
  std::vector<DeviceInfo> devs = {cpu, cpu};  // two logical CPU devices
  CoresConfig cfg;
  Cores cores(devs, kSrc, cfg);
  CHECK(cores.error_code() == 0);
  if (cores.error_code()) {
    std::fprintf(stderr, "%s\n", cores.error_message().c_str());
    return;
  }
  const long long n = 64 * 64;
  std::vector<float> a(1, 3.0f), x(n), y(n, 1.0f);
  for (long long i = 0; i < n; ++i) x[i] = static_cast<float>(i % 97);

  // plain + event pipeline + driver pipeline
  for (int mode = 0; mode < 3; ++mode) {
    std::fill(y.begin(), y.end(), 1.0f);
    ComputeCall c;
    c.kernels = {"saxpy"};
    ArraySpec sa = spec(1, a.data(), 4, 4), sx = spec(2, x.data(), n * 4, 4), sy = spec(3, y.data(), n * 4, 4);
    sa.write = false;
    sx.write = false;
    sx.partial = mode > 0;
    sy.partial = mode > 0;
    c.arrays = {sa, sx, sy};
    c.global_range = n;
    c.local_range = 64;
    c.compute_id = 10 + mode;
    c.pipeline = mode > 0;
    c.pipeline_event = mode == 1;
    c.blobs = 4;
    cores.record_schedule = true;
    for (int it = 0; it < 3; ++it) {
      std::fill(y.begin(), y.end(), 1.0f);
      cores.compute(c);
    }
    for (long long i = 0; i < n; ++i) CHECK(y[i] == 3.0f * x[i] + 1.0f);
  }
  CHECK(!cores.schedule().empty());

  // repeat + sync kernel
  {
    std::vector<float> v(1024, 0.0f);
    std::vector<int> cnt(1, 0);
    ComputeCall c;
    c.kernels = {"incc"};
    c.repeats = 5;
    c.repeat_kernel = "count";
    ArraySpec sv = spec(4, v.data(), v.size() * 4, 4), sc = spec(5, cnt.data(), 4, 4);
    sc.write_all = true;
    c.arrays = {sv, sc};
    c.global_range = 1024;
    c.local_range = 64;
    c.compute_id = 20;
    cores.compute(c);
    for (float f : v) CHECK(f == 5.0f);
  }

  // barrier kernel (fibers) with per-group outputs
  {
    std::vector<float> v(n), out(n / 64, 0.0f);
    for (long long i = 0; i < n; ++i) v[i] = 1.0f;
    ComputeCall c;
    c.kernels = {"groupsum"};
    ArraySpec sv = spec(6, v.data(), n * 4, 4), so = spec(7, out.data(), out.size() * 4, 4);
    sv.write = false;
    so.read = false;
    so.epg = 1;
    c.arrays = {sv, so};
    c.global_range = n;
    c.local_range = 64;
    c.compute_id = 21;
    cores.compute(c);
    for (float f : out) CHECK(f == 64.0f);
  }

  // arity mismatch is rejected before any launch
  {
    std::vector<float> v(256, 0.0f);
    std::vector<int> cnt(1, 0);
    ComputeCall c;
    c.kernels = {"inc"};
    ArraySpec sv = spec(8, v.data(), 1024, 4), sc = spec(9, cnt.data(), 4, 4);
    sc.write = false;
    c.arrays = {sv, sc};
    c.global_range = 256;
    c.local_range = 64;
    bool threw = false;
    try {
      cores.compute(c);
    } catch (const std::exception&) {
      threw = true;
    }
    CHECK(threw);
  }

  // failover: device 1 fails once, its slice is recomputed on device 0
  {
    std::vector<float> v(1024, 0.0f);
    ComputeCall c;
    c.kernels = {"inc"};
    c.arrays = {spec(10, v.data(), v.size() * 4, 4)};
    c.global_range = 1024;
    c.local_range = 64;
    c.compute_id = 22;
    cores.auto_failover = true;
    cores.inject_failure(1, 1);
    cores.compute(c);
    for (float f : v) CHECK(f == 1.0f);
    CHECK(!cores.device_enabled(1) && cores.failovers() == 1);
    cores.set_device_enabled(1, true);
  }
  cores.finish();
}

int main() {
  test_balancer();
  test_jit();
  test_byte_chunk();
  test_lane_ids();
  test_job_thread();
  test_cpu_worker_parts();
  test_cores();
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("runtime self-test passed\n");
  return 0;
}
