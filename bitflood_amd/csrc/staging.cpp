// staging.cpp -- the pipeline that moves a job's chunks from host memory or
// files into device slots and their results back: slots, the copy pool, the
// direct and staged copy routes, and worker_run, which drives one worker's
// batches.  What goes where in a batch is decided by stage_plan.hpp.
#include <hip/hip_runtime.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <functional>
#include <thread>

#include "lbf_host.hpp"

namespace lbf {

unsigned copy_threads() {
  static const unsigned n = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(64, env_u64("LBF_COPY_THREADS", 8)));
  return n;
}

uint64_t Source::read_serial(uint8_t* dst, uint32_t file, uint64_t off, uint64_t len) const {
  if (!from_files()) {
    memcpy(dst, base + off, len);
    return len;
  }
  const int fd = fds[file];
  uint64_t got = 0;
  while (fd >= 0 && got < len) {
    const ssize_t r = pread(fd, dst + got, len - got, (off_t)(off + got));
    if (r <= 0) break;  // EOF or error: the rest is unavailable
    got += (uint64_t)r;
  }
  return got;
}

// Helper threads of one worker's staging copies, started once and kept: a
// staging piece (LBF_PIN_MB, 128 MiB) moves in ≈2.5 ms at PCIe rate, and
// starting, binding and joining seven threads for every piece cost a
// measurable share of that (threads per call: 40 against 46-50 GiB/s,
// DESIGN.md §5).  run() hands the helpers a piece count and a function, joins
// in itself, and returns once every helper is done with it.
class CopyPool {
 public:
  CopyPool(unsigned helpers, const std::vector<int>& cpus) {
    for (unsigned t = 0; t < helpers; ++t) {
      try {
        th_.emplace_back([this, cpus] {
          bind_thread(cpus);
          loop();
        });
      } catch (const std::system_error&) {
        break;  // fewer helpers: the caller and the others take their pieces
      }
    }
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lock(mu_);
      stop_ = true;
    }
    cv_work_.notify_all();
    for (std::thread& t : th_) t.join();
  }
  CopyPool(const CopyPool&) = delete;
  CopyPool& operator=(const CopyPool&) = delete;

  size_t helpers() const { return th_.size(); }

  // fn(q) for q in [0, n), spread over the caller and the helpers
  void run(size_t n, const std::function<void(size_t)>& fn) {
    {
      std::lock_guard<std::mutex> lock(mu_);
      fn_ = &fn;
      n_ = n;
      next_.store(0);
      busy_ = th_.size();
      ++gen_;
    }
    cv_work_.notify_all();
    pull(fn, n);
    std::unique_lock<std::mutex> lock(mu_);
    cv_done_.wait(lock, [this] { return busy_ == 0; });
    fn_ = nullptr;
  }

 private:
  void pull(const std::function<void(size_t)>& fn, size_t n) {
    for (size_t q; (q = next_++) < n;) fn(q);
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      const std::function<void(size_t)>* fn;
      size_t n;
      {
        std::unique_lock<std::mutex> lock(mu_);
        cv_work_.wait(lock, [&] { return stop_ || gen_ != seen; });
        if (stop_) return;
        seen = gen_;
        fn = fn_;
        n = n_;
      }
      pull(*fn, n);
      std::lock_guard<std::mutex> lock(mu_);
      if (--busy_ == 0) cv_done_.notify_one();
    }
  }

  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_work_, cv_done_;
  const std::function<void(size_t)>* fn_ = nullptr;
  size_t n_ = 0;
  std::atomic<size_t> next_{0};
  size_t busy_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

namespace {

constexpr uint64_t kHdrAlign = 256;
constexpr uint64_t kDescBytes = 8 + 4 + 20;

uint64_t header_bytes(uint64_t cnt) { return (cnt * kDescBytes + kHdrAlign - 1) / kHdrAlign * kHdrAlign; }

// Pinned host memory on the worker's NUMA node (hipHostMallocNumaUser makes
// the allocation follow the calling thread's memory policy).  Allocations and
// frees of pinned memory pass one process-wide mutex.  The HIP runtime is
// thread-safe on its own; the mutex makes a context's teardown visibly happen
// before another context reuses the same pinned pages, which is what a
// ThreadSanitizer build (tools/tsan_build.sh) needs to see: it cannot look
// inside the uninstrumented runtime's allocator, and reported the reuse of a
// destroyed context's pages by the next one as a race.
std::mutex g_pinned_mu;

hipError_t host_alloc(const Worker& w, void** p, uint64_t bytes) {
  if (w.numa_node >= 0) {
    PreferNode pref(w.numa_node);
    if (pref.active) {
      std::lock_guard<std::mutex> lock(g_pinned_mu);
      return hipHostMalloc(p, bytes, hipHostMallocNumaUser);
    }
  }
  std::lock_guard<std::mutex> lock(g_pinned_mu);
  return hipHostMalloc(p, bytes, hipHostMallocDefault);
}

void host_free(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lock(g_pinned_mu);
  (void)hipHostFree(p);  // release paths: a failure has nowhere to go
}

// An on-the-fly registration pins only the pages that lie wholly inside the
// job's bytes (pin_on_the_fly), so a direct batch may hold up to a page at
// each end of the job that is not pinned: those bytes are bounced through
// this much pinned memory per device slot.
uint64_t edge_cap() { return 2 * (uint64_t)sysconf(_SC_PAGESIZE); }

int dev_slot_init(Worker& w, DevSlot& d) {
  LBF_HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  LBF_HIP_TRY(hipMalloc((void**)&d.d_out, w.desc_cap * 20));
  LBF_HIP_TRY(host_alloc(w, (void**)&d.h_out, w.desc_cap * 20));
  LBF_HIP_TRY(host_alloc(w, (void**)&d.h_hdr, w.hdr_cap));
  LBF_HIP_TRY(host_alloc(w, (void**)&d.h_edge, edge_cap()));
  if (w.slot_bytes) LBF_HIP_TRY(hipMalloc((void**)&d.d_buf, w.hdr_cap + w.slot_bytes));
  LBF_HIP_TRY(hipEventCreateWithFlags(&d.copied, hipEventDisableTiming));
  d.ok.assign(w.desc_cap, 0);
  return LBF_OK;
}

void dev_slot_free(DevSlot& d) {
  // errors here have nowhere to go: the slot is being released
  if (d.stream) (void)hipStreamSynchronize(d.stream);
  if (d.d_buf) (void)hipFree(d.d_buf);
  if (d.d_out) (void)hipFree(d.d_out);
  host_free(d.h_out);
  host_free(d.h_hdr);
  host_free(d.h_edge);
  if (d.copied) (void)hipEventDestroy(d.copied);
  if (d.stream) (void)hipStreamDestroy(d.stream);
  d = DevSlot{};
}

// Staging memory is sized to the work, not reserved up front: pinning 2 x 512
// MiB costs ≈200 ms at context creation and ≈110 ms at destruction
// (tools/startup_probe.py), which a one-chunk Base64Encode or a small file
// should not pay.  Slots grow, never shrink, in 8 MiB steps up to slot_max.
constexpr uint64_t kSlotStep = 8ull << 20;

int ensure_slot_bytes(Worker& w, uint64_t need, uint64_t dev_cap) {
  auto round = [](uint64_t x, uint64_t cap) {
    return std::min(cap, (std::max(x, kSlotStep) + kSlotStep - 1) / kSlotStep * kSlotStep);
  };
  const uint64_t dev_need = round(need, dev_cap);
  const uint64_t pin_need = round(std::min(need, w.pin_max), w.pin_max);
  if (dev_need > w.slot_bytes) {
    for (DevSlot& d : w.dev) {
      LBF_HIP_TRY(hipStreamSynchronize(d.stream));
      if (d.d_buf) (void)hipFree(d.d_buf);
      d.d_buf = nullptr;
    }
    w.slot_bytes = 0;
    for (DevSlot& d : w.dev) LBF_HIP_TRY(hipMalloc((void**)&d.d_buf, w.hdr_cap + dev_need));
    w.slot_bytes = dev_need;
  }
  if (pin_need > w.pin_bytes) {
    for (DevSlot& d : w.dev) LBF_HIP_TRY(hipStreamSynchronize(d.stream));  // no H2D reads a host slot
    for (HostSlot& h : w.host) {
      host_free(h.h_buf);
      h.h_buf = nullptr;
      h.in_flight = false;
    }
    w.pin_bytes = 0;
    for (HostSlot& h : w.host) LBF_HIP_TRY(host_alloc(w, (void**)&h.h_buf, pin_need));
    w.pin_bytes = pin_need;
  }
  return LBF_OK;
}

// Device slots for a job whose longest staged chunk is `largest` bytes: enough
// to keep ≈50 GB/s of H2D going for one chain's duration
// (chain_bytes_in_flight), never more than the process's hardware queues
// (GPU_MAX_HW_QUEUES, HIP's default 4): streams beyond that share a queue, and
// a batch's copies would then wait behind another slot's long kernel.  At
// least kDevSlots, at most the HBM budget.
constexpr uint64_t kDevSlots = 3;

int ensure_dev_slots(Worker& w, uint64_t largest, uint64_t groups) {
  static const uint64_t hw_queues = (uint64_t)std::max(2L, std::min(32L, env_long("GPU_MAX_HW_QUEUES", 4)));
  const uint64_t in_flight = chain_bytes_in_flight(largest);
  const uint64_t per = w.hdr_cap + w.slot_bytes;
  uint64_t want = (in_flight + w.slot_bytes - 1) / std::max<uint64_t>(1, w.slot_bytes) + 1;
  want = std::min<uint64_t>(want, groups);
  want = std::min<uint64_t>(want, std::max<uint64_t>(1, w.dev_budget / per));
  want = std::min<uint64_t>(hw_queues, std::max<uint64_t>(want, std::min(kDevSlots, hw_queues)));
  while (w.dev.size() < want) {
    w.dev.emplace_back();
    if (int rc = dev_slot_init(w, w.dev.back())) {
      std::string msg = lbf_last_error();
      dev_slot_free(w.dev.back());
      w.dev.pop_back();
      if (w.dev.size() >= kDevSlots) break;  // fewer slots in flight: slower, not wrong
      return fail(rc, msg);
    }
  }
  return LBF_OK;
}

// After a job, give back the device slots beyond kDevSlots, and the HBM of
// batches grown past LBF_SLOT_MB for long chains (the next job sizes its own).
void trim_dev_slots(Worker& w) {
  while (w.dev.size() > kDevSlots) {
    dev_slot_free(w.dev.back());
    w.dev.pop_back();
  }
  if (w.slot_bytes > w.slot_max) {
    for (DevSlot& d : w.dev) {
      (void)hipStreamSynchronize(d.stream);  // drained already; errors were reported by the job
      if (d.d_buf) (void)hipFree(d.d_buf);
      d.d_buf = nullptr;
    }
    w.slot_bytes = 0;
  }
}

}  // namespace

int worker_init(Worker& w, int device, int index) {
  w.device = device;
  w.index = index;
  w.slot_max = std::max<uint64_t>(env_u64("LBF_SLOT_MB", 512) << 20, 1ull << 20);
  w.pin_max = std::max<uint64_t>(env_u64("LBF_PIN_MB", 128) << 20, 1ull << 20);
  w.dev_budget = std::max<uint64_t>(env_u64("LBF_DEVICE_STAGING_MB", 16384) << 20, 1ull << 20);
  // Three pinned slots keep the PCIe link busy: with two, staging group g+2
  // waits for group g's H2D, so the link idles while the host copies.
  w.host.resize(std::min<uint64_t>(8, std::max<uint64_t>(2, env_u64("LBF_SLOTS", 3))));
  w.slot_bytes = 0;
  w.desc_cap = 1u << 16;
  w.hdr_cap = header_bytes(w.desc_cap);
  // Test hook: fail the g-th group this worker stages (once), after earlier
  // groups are in flight, to exercise the drain on the error path.
  if (env_long("LBF_TEST_FAULT_WORKER", 0) == index) w.fault_group = env_long("LBF_TEST_FAULT_GROUP", -1);
  const char* kind = getenv("LBF_TEST_FAULT_KIND");
  w.fault_throws = kind && strcmp(kind, "throw") == 0;
  LBF_HIP_TRY(hipSetDevice(device));
  if (numa_enabled()) {
    w.numa_node = device_numa_node(device);
    w.cpus = node_cpus_allowed(w.numa_node);
  }
  for (HostSlot& h : w.host) LBF_HIP_TRY(hipEventCreateWithFlags(&h.copied, hipEventDisableTiming));
  w.dev.resize(kDevSlots);
  for (DevSlot& d : w.dev)
    if (int rc = dev_slot_init(w, d)) return rc;
  return LBF_OK;
}

void worker_free(Worker& w) {
  w.pool.reset();  // idle between jobs: the helpers only need waking and joining
  if (hipSetDevice(w.device) != hipSuccess) return;
  // teardown: errors here have nowhere to go, the context is being destroyed
  for (DevSlot& d : w.dev) dev_slot_free(d);
  w.dev.clear();
  for (HostSlot& h : w.host) {
    host_free(h.h_buf);
    if (h.copied) (void)hipEventDestroy(h.copied);
    h = HostSlot{};
  }
}

namespace {

// Copy every run of a group into the slot's data area.  A single host thread
// copies ~17 GiB/s into pinned memory, a third of what PCIe Gen5 moves, so
// runs are cut into pieces of at most `step` bytes (≥ 8 MiB of work per
// thread; `step` rounded up to a page) that the caller and the worker's
// CopyPool helpers, bound to the staging's NUMA node, pull from a shared
// index: one long contiguous run and many small scattered ones copy in
// parallel alike.  (The ceil(total / parts) step must cover everything:
// rounding floor(len / parts) once left the last bytes of a range uncopied,
// tools/fuzz_gpu.py seed 23006099, pinned by test_staging_split_covers_tail.)
void read_runs(const Source& src, std::vector<Run>& runs, uint8_t* data, Worker& w) {
  constexpr uint64_t kMinPart = 8ull << 20;
  uint64_t total = 0;
  for (const Run& r : runs) total += r.len;
  const uint64_t parts = std::min<uint64_t>(src.threads, total / kMinPart);
  if (parts <= 1) {
    for (Run& r : runs) r.avail = src.read_serial(data + r.dst, r.file, r.src, r.len);
    return;
  }
  const uint64_t step = ((total + parts - 1) / parts + 4095) & ~4095ull;
  struct Piece {
    size_t run;
    uint64_t at, len, got;
  };
  std::vector<Piece> pieces;
  for (size_t k = 0; k < runs.size(); ++k)
    for (uint64_t a = 0; a < runs[k].len; a += step) pieces.push_back({k, a, std::min(step, runs[k].len - a), 0});
  const std::function<void(size_t)> copy = [&](size_t q) {
    Piece& pc = pieces[q];
    pc.got = src.read_serial(data + runs[pc.run].dst + pc.at, runs[pc.run].file, runs[pc.run].src + pc.at, pc.len);
  };
  // the worker's helpers (copy_threads() - 1 of them, bound to its node) plus
  // the calling thread, already bound by its worker
  if (!w.pool) w.pool = std::make_shared<CopyPool>(copy_threads() - 1, w.cpus);
  w.pool->run(pieces.size(), copy);
  // a run's readable prefix: its pieces in order up to the first short one
  std::vector<bool> short_seen(runs.size(), false);
  for (Run& r : runs) r.avail = 0;
  for (const Piece& pc : pieces) {
    if (short_seen[pc.run]) continue;
    runs[pc.run].avail += pc.got;
    if (pc.got < pc.len) short_seen[pc.run] = true;
  }
}

int io_error(uint64_t chunk) {
  return fail(LBF_ERR_IO, "chunk " + std::to_string(chunk) + " could not be read in full");
}

// Copy finished results of a slot's group (positions [g_begin, g_end)) to the
// caller's arrays.  Chunks that were not fully readable: verdict 0 (verify) or
// an LBF_ERR_IO (hash).
int finalize(const Job& job, const Order& order, DevSlot& s) {
  if (!s.pending) return LBF_OK;
  s.pending = false;
  const uint64_t cnt = s.g_end - s.g_begin;
  if (job.expected) {
    for (uint64_t k = 0; k < cnt; ++k) job.verdicts[order(s.g_begin + k)] = s.h_out[k] & s.ok[k];
    return LBF_OK;
  }
  for (uint64_t k = 0; k < cnt; ++k)
    if (!s.ok[k]) return io_error(order(s.g_begin + k));
  if (order.perm.empty()) {
    memcpy(job.digests + 20 * s.g_begin, s.h_out, cnt * 20);
  } else {
    for (uint64_t k = 0; k < cnt; ++k) memcpy(job.digests + 20 * order(s.g_begin + k), s.h_out + 20 * k, 20);
  }
  return LBF_OK;
}

// One chunk that does not fit a slot: a dedicated device buffer, synchronous
// (device slot 0's stream and host slot 0's header, both idle by then).
int run_oversize(Worker& w, const Job& job, uint64_t i) {
  DevSlot& s = w.dev[0];
  HostSlot& h = w.host[0];
  LBF_HIP_TRY(hipStreamSynchronize(s.stream));
  const uint32_t sz = job.sizes[i];
  std::vector<uint8_t> host(sz ? sz : 1);
  std::vector<Run> one{Run{job.offsets[i], sz, 0, 0, job.file(i)}};
  read_runs(job.src, one, host.data(), w);
  // header of a one-chunk group: offset 0, size sz, expected digest
  const HeaderEntry e = header_entry(&one[0], job.src.exists(job.file(i)), job.offsets[i], sz);
  if (!e.ok) {
    if (!job.expected) return io_error(i);
    job.verdicts[i] = 0;
    return LBF_OK;
  }
  uint8_t* d = nullptr;
  LBF_HIP_TRY(hipMalloc((void**)&d, sz ? sz : 1));
  int rc = LBF_OK;
  do {
    memcpy(h.h_buf, &e.off, 8);
    memcpy(h.h_buf + 8, &e.size, 4);
    if (job.expected) memcpy(h.h_buf + 12, job.expected + 20 * i, 20);
    if (hipMemcpy(d, host.data(), sz, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s.d_buf, h.h_buf, kDescBytes, hipMemcpyHostToDevice) != hipSuccess) {
      rc = fail(LBF_ERR_HIP, "oversize chunk H2D failed");
      break;
    }
    const uint64_t* d_off = reinterpret_cast<const uint64_t*>(s.d_buf);
    const uint32_t* d_size = reinterpret_cast<const uint32_t*>(s.d_buf + 8);
    rc = lbf_sha1_launch(d, d_off, d_size, 1, job.expected ? nullptr : s.d_out, job.expected ? s.d_buf + 12 : nullptr,
                         job.expected ? s.d_out : nullptr, s.stream);
    if (rc) break;
    if (hipStreamSynchronize(s.stream) != hipSuccess) {
      rc = fail(LBF_ERR_HIP, "oversize kernel failed");
      break;
    }
    const hipError_t err = job.expected ? hipMemcpy(job.verdicts + i, s.d_out, 1, hipMemcpyDeviceToHost)
                                        : hipMemcpy(job.digests + 20 * i, s.d_out, 20, hipMemcpyDeviceToHost);
    if (err != hipSuccess) rc = fail(LBF_ERR_HIP, "oversize D2H failed");
  } while (0);
  (void)hipFree(d);
  return rc;
}

// A registered (pinned) source goes to the device without the staging copy,
// one H2D per run, when its group's runs average at least kDirectMinRun:
// below that, per-copy overhead costs more than the host memcpy it saves.
// Measured on one MI355X (tools/e2e_sizes.py --register), with
// each batch's copies ordered after the previous batch's (stage_direct): 14.4
// against 12.0-12.5 GiB/s staged at 64 MiB, 44.4-45.1 against 29.5-42.8 at
// 1 GiB, 49.6-50.6 against 33.6-49.5 at 4 GiB.  Every job size goes direct.
constexpr uint64_t kDirectMinRun = 1ull << 20;

// One worker_run call: the job, its order, and where the pipeline stands.
// A failed step leaves its status in rc; the driver stops at the first one.
struct Batch {
  const Job& job;
  Order order;
  Group g;               // the group being staged
  int cur = 0;           // device slot of the group being staged
  int hcur = 0;          // next host slot
  int prev_direct = -1;  // device slot of the last direct-route batch
  long group = 0;        // groups staged so far (LBF_TEST_FAULT_GROUP counts them)
  int rc = LBF_OK;

  bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    rc = hip_fail(e, what);
    return false;
  }
};

// Step 1: size the job's slots (stage_plan.hpp, size_job) and grow the rings.
int size_and_grow(Worker& w, const Batch& b, uint64_t begin, uint64_t end) {
  if (end <= begin) return LBF_OK;
  const JobSize js = size_job(b.job, b.order, begin, end, w.slot_max, w.dev_budget);
  // (LBF_SLOT_MB stays the cap unless the long-chain rule raised the batch)
  if (int rc = ensure_slot_bytes(w, js.per + 16, js.per > w.slot_max ? js.dev_cap : w.slot_max)) return rc;
  const uint64_t groups = js.bytes / std::max<uint64_t>(1, w.slot_bytes) + 2;
  return ensure_dev_slots(w, js.largest, groups);
}

// Step 3: the slot's previous group is done; hand its results to the caller.
void wait_and_finalize(Batch& b, DevSlot& s) {
  if (b.hip_ok(hipStreamSynchronize(s.stream), "hipStreamSynchronize")) b.rc = finalize(b.job, b.order, s);
}

// A chunk that fits no slot runs alone, after everything in flight.
void oversize_step(Worker& w, Batch& b) {
  for (DevSlot& s : w.dev) {
    wait_and_finalize(b, s);
    if (b.rc) return;
  }
  b.rc = run_oversize(w, b.job, b.order(b.g.begin));
}

// The H2D copies of one direct batch.  A run's bytes outside the pinned pages
// (an on-the-fly span's first and last partial page, AutoPin) go through the
// slot's pinned bounce: the slot's stream is idle here, so its previous
// contents are spent.  Bytes that do not fit it send the batch through staging.
struct DirectCopies {
  Worker& w;
  Batch& b;
  DevSlot& s;
  uint64_t pin_lo, pin_hi;  // the pinned pages, as source offsets
  uint64_t bounced = 0;
  bool refused = false;  // a copy HIP refuses from an on-the-fly registration (see below)

  bool ok() const { return b.rc == LBF_OK && !refused; }

  void copy(uint64_t dst, uint64_t src, uint64_t len) {  // one H2D of source bytes [src, src + len)
    const Source& source = b.job.src;
    const uint8_t* from = source.base + src;
    if (src < pin_lo || src + len > pin_hi) {
      if (bounced + len > edge_cap()) {
        refused = true;
        return;
      }
      memcpy(s.h_edge + bounced, from, len);
      from = s.h_edge + bounced;
      bounced += len;
    }
    const hipError_t e = hipMemcpyAsync(s.d_buf + w.hdr_cap + dst, from, len, hipMemcpyHostToDevice, s.stream);
    if (e == hipErrorInvalidValue && source.autopinned) {
      // HIP lets a span be registered over a range the caller had
      // pinned itself, then resolves copies in that range to the
      // caller's (smaller) registration and refuses them at enqueue.
      // Such a batch is staged; the copies already queued run before
      // the staged ones on the same stream, which overwrite whatever
      // they wrote.
      (void)hipGetLastError();
      refused = true;
    } else {
      b.hip_ok(e, "hipMemcpyAsync(H2D, registered source)");
    }
  }
};

// Step 4, direct route: each run is copied to the device straight from the
// caller's pinned memory.  Returns true when the batch went direct; false
// with rc clear when HIP refused it and it must be staged.  `edge_bytes`: what
// passed through the bounce.
bool stage_direct(Worker& w, Batch& b, DevSlot& s, uint64_t& edge_bytes) {
  // A batch's copies start only once the previous direct batch's have
  // landed.  Issued freely, the copies of every batch in the ring shared
  // the link, all batches finished copying together, and the link then
  // sat idle through their kernels (rocprofv3 trace,
  // profiles/r02/registered_trace/direct_ordered/).  In order, batch g
  // is hashed while batch g+1 is still copying, as on the staged route.
  if (b.prev_direct >= 0 && b.prev_direct != b.cur &&
      !b.hip_ok(hipStreamWaitEvent(s.stream, w.dev[b.prev_direct].copied, 0), "hipStreamWaitEvent"))
    return false;
  // One copy per run.  Before the copies were ordered, 32 MiB pieces helped (4 GiB 42.5 -> 47.2
  // GiB/s, profiles/r02/registered_trace/piece_sweep/); ordered, whole runs are as fast
  // or faster (50.6 against 49.6-49.8 GiB/s at 4 GiB, direct_ordered/).
  const uintptr_t base = reinterpret_cast<uintptr_t>(b.job.src.base);
  DirectCopies c{w, b, s, b.job.src.pin_lo - base, b.job.src.pin_hi - base};
  for (Run& r : b.g.runs) {
    // [r.src, r.src + r.len) cut at the pinned pages' ends: head, body, tail
    const uint64_t end = r.src + r.len;
    const uint64_t b0 = std::min(std::max(r.src, c.pin_lo), end), b1 = std::max(std::min(end, c.pin_hi), b0);
    if (b0 > r.src) c.copy(r.dst, r.src, b0 - r.src);
    if (b1 > b0 && c.ok()) c.copy(r.dst + (b0 - r.src), b0, b1 - b0);
    if (end > b1 && c.ok()) c.copy(r.dst + (b1 - r.src), b1, end - b1);
    if (!c.ok()) break;
    r.avail = r.len;
  }
  edge_bytes = c.refused ? 0 : c.bounced;
  if (b.rc) return false;
  if (c.refused) {
    for (Run& r : b.g.runs) r.avail = 0;
    return false;
  }
  if (!b.hip_ok(hipEventRecord(s.copied, s.stream), "hipEventRecord")) return false;
  b.prev_direct = b.cur;
  return true;
}

// The next host slot, once its last H2D is done (null: rc is set).
HostSlot* free_host_slot(Worker& w, Batch& b) {
  HostSlot& h = w.host[b.hcur];
  if (h.in_flight && !b.hip_ok(hipEventSynchronize(h.copied), "hipEventSynchronize")) return nullptr;
  h.in_flight = false;
  return &h;
}

// Step 4, staged route, a batch larger than a host slot: pieces of pin_bytes
// through the host ring, one H2D each (the header follows from the slot's own
// pinned header buffer).
void stage_pieces(Worker& w, Batch& b, DevSlot& s) {
  PieceCutter cutter(b.g.runs.size());
  for (uint64_t pstart = 0; pstart < b.g.cursor;) {
    const uint64_t pend = std::min(b.g.cursor, pstart + w.pin_bytes);
    HostSlot* h = free_host_slot(w, b);
    if (!h) return;
    cutter.cut(b.g.runs, pstart, pend);
    read_runs(b.job.src, cutter.parts, h->h_buf, w);
    cutter.fold(b.g.runs);
    if (!b.hip_ok(hipMemcpyAsync(s.d_buf + w.hdr_cap + pstart, h->h_buf, pend - pstart, hipMemcpyHostToDevice, s.stream),
                  "hipMemcpyAsync(H2D)") ||
        !b.hip_ok(hipEventRecord(h->copied, s.stream), "hipEventRecord"))
      return;
    h->in_flight = true;
    b.hcur = (b.hcur + 1) % (int)w.host.size();
    pstart = pend;
  }
}

// Step 5: the header of the group at h_header (stage_plan.hpp, header_entry).
void write_header(const Batch& b, DevSlot& s, uint8_t* h_header) {
  const Job& job = b.job;
  const uint64_t cnt = b.g.end - b.g.begin;
  uint64_t* h_off = reinterpret_cast<uint64_t*>(h_header);
  uint32_t* h_size = reinterpret_cast<uint32_t*>(h_header + 8 * cnt);
  uint8_t* h_exp = h_header + 12 * cnt;
  for (uint64_t q = 0; q < cnt; ++q) {
    const uint64_t k = b.order(b.g.begin + q);
    const uint32_t r = b.g.run_of[q];
    const HeaderEntry e = header_entry(r == UINT32_MAX ? nullptr : &b.g.runs[r], job.src.exists(job.file(k)),
                                       job.offsets[k], job.sizes[k]);
    s.ok[q] = e.ok ? 1 : 0;
    h_off[q] = e.off;
    h_size[q] = e.size;
    if (job.expected) memcpy(h_exp + 20 * q, job.expected + 20 * k, 20);
  }
}

// Step 6: header (+ data, for a single-piece batch) after the pieces, on the
// same stream; then the kernel and the D2H of its results.
void submit(Worker& w, Batch& b, DevSlot& s, const uint8_t* h_header, bool single) {
  const Job& job = b.job;
  const uint64_t cnt = b.g.end - b.g.begin, hdr = header_bytes(cnt);
  const uint64_t data_off = single ? hdr : w.hdr_cap;
  const uint64_t bytes = single ? hdr + b.g.cursor : hdr;
  if (!b.hip_ok(hipMemcpyAsync(s.d_buf, h_header, bytes, hipMemcpyHostToDevice, s.stream), "hipMemcpyAsync(H2D)")) return;
  if (single) {
    HostSlot& h = w.host[b.hcur];
    if (!b.hip_ok(hipEventRecord(h.copied, s.stream), "hipEventRecord")) return;
    h.in_flight = true;
    b.hcur = (b.hcur + 1) % (int)w.host.size();
  }
  const uint64_t* d_off = reinterpret_cast<const uint64_t*>(s.d_buf);
  const uint32_t* d_size = reinterpret_cast<const uint32_t*>(s.d_buf + 8 * cnt);
  if (job.expected)
    b.rc = lbf_sha1_launch(s.d_buf + data_off, d_off, d_size, cnt, nullptr, s.d_buf + 12 * cnt, s.d_out, s.stream);
  else b.rc = lbf_sha1_launch(s.d_buf + data_off, d_off, d_size, cnt, s.d_out, nullptr, nullptr, s.stream);
  if (b.rc) return;
  if (!b.hip_ok(hipMemcpyAsync(s.h_out, s.d_out, cnt * (job.expected ? 1 : 20), hipMemcpyDeviceToHost, s.stream),
                "hipMemcpyAsync(D2H)"))
    return;
  s.pending = true;
  s.g_begin = b.g.begin;
  s.g_end = b.g.end;
}

// Step 4 for the packed group b.g on device slot s.  The batch's bytes,
// [0, cursor) of its data area, go through the host ring: in one
// [header | data] copy when they fit a host slot (`single`; the copy is
// submit's), else in pieces (stage_pieces).  A registered source skips the
// ring (stage_direct).  Returns where the batch's header is to be written.
uint8_t* stage_group(Worker& w, Batch& b, DevSlot& s, bool& single) {
  const uint64_t cursor = b.g.cursor, hdr = header_bytes(b.g.end - b.g.begin);
  bool direct = b.job.src.pinned && !b.g.runs.empty() && cursor >= b.g.runs.size() * kDirectMinRun;
  uint64_t edge_bytes = 0;
  for (Run& r : b.g.runs) r.avail = 0;
  if (direct) direct = stage_direct(w, b, s, edge_bytes);
  if (b.rc) return nullptr;
  single = !direct && hdr + cursor <= w.pin_bytes;
  // (a direct batch's bounced edge bytes count as staged: they took a host copy)
  (direct ? w.bytes_direct : w.bytes_staged) += cursor - edge_bytes;
  w.bytes_staged += edge_bytes;
  uint8_t* h_header = s.h_hdr;
  if (single) {
    // the header is written next to the data, then header + data go in one copy
    HostSlot* h = free_host_slot(w, b);
    if (!h) return nullptr;
    read_runs(b.job.src, b.g.runs, h->h_buf + hdr, w);
    h_header = h->h_buf;
  } else if (!direct) {
    stage_pieces(w, b, s);
  }
  return h_header;
}

// Step 7: the drain, on every path (every H2D ran on a device slot's stream,
// so this also completes every host slot's copy).
int drain(Worker& w, Batch& b) {
  int rc = b.rc;
  for (DevSlot& s : w.dev) {
    const hipError_t e = hipStreamSynchronize(s.stream);
    if (e != hipSuccess && rc == LBF_OK) rc = hip_fail(e, "hipStreamSynchronize");
    if (rc == LBF_OK) rc = finalize(b.job, b.order, s);
    s.pending = false;
  }
  for (HostSlot& h : w.host) h.in_flight = false;
  trim_dev_slots(w);
  return rc;
}

// Process descriptors [begin, end) on one worker.  They are staged in source
// order and packed into groups of runs (stage_plan.hpp).  One H2D per group
// (or per piece, or per run on the direct route), one kernel, one D2H; the
// host stages group g+1 while the GPU works on the groups before it.  The
// steps, numbered below: 1 size the job and grow the slots, then per group
// 2 pack, 3 wait for the slot and finalize, 4 stage, 5 write the header,
// 6 submit; 7 drain.
//
// Every exit, error or not, passes the drain at the end: each slot's stream is
// synchronized and its pending group cleared, so nothing is still in flight
// and no stale group can be finalized into the next job's arrays.
int worker_run(Worker& w, const Job& job, uint64_t begin, uint64_t end) {
  LBF_HIP_TRY(hipSetDevice(w.device));
  Batch b{job, source_order(job, begin, end)};
  if (int rc = size_and_grow(w, b, begin, end)) return rc;  // 1
  // An exception in the loop (a host allocation) must not skip the drain
  // below: groups may be in flight.
  try {
    for (uint64_t i = begin; i < end && b.rc == LBF_OK; i = b.g.end) {
      pack_group(job, b.order, i, end, w.slot_bytes, w.desc_cap, b.g);  // 2
      if (b.g.oversize) {
        oversize_step(w, b);
        continue;
      }
      DevSlot& s = w.dev[b.cur];
      wait_and_finalize(b, s);  // 3
      if (b.rc) break;
      if (b.group++ == w.fault_group) {
        w.fault_group = -1;
        if (w.fault_throws) throw std::bad_alloc();  // must still reach the drain
        b.rc = fail(LBF_ERR_HIP, "injected fault (LBF_TEST_FAULT_GROUP) at group " + std::to_string(b.group - 1));
        break;
      }
      bool single = false;
      uint8_t* h_header = stage_group(w, b, s, single);  // 4
      if (b.rc) break;
      write_header(b, s, h_header);             // 5
      submit(w, b, s, h_header, single);        // 6
      if (b.rc) break;
      b.cur = (b.cur + 1) % (int)w.dev.size();
    }
  } catch (const std::bad_alloc&) {
    b.rc = fail(LBF_ERR_NOMEM, "host allocation failed while staging");
  } catch (const std::system_error& e) {
    b.rc = fail(LBF_ERR_NOMEM, std::string("host resources while staging: ") + e.what());
  } catch (const std::exception& e) {
    b.rc = fail(LBF_ERR_INVALID, std::string("internal error while staging: ") + e.what());
  }
  return drain(w, b);  // 7
}

}  // namespace

// Contiguous index ranges per worker, one host thread each (bound to its
// worker's NUMA node), no collective.
int run_job(lbf_ctx* ctx, Job job, uint64_t n) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  KeepCurrentDevice keep;  // worker 0 (and any inline worker) runs on this thread
  if (!job.src.from_files() && in_registered(ctx, job.src.base, job.src.base_len)) {
    job.src.pinned = true;
    job.src.pin_lo = reinterpret_cast<uintptr_t>(job.src.base);
    job.src.pin_hi = job.src.pin_lo + job.src.base_len;
  }
  // Declared before the workers run and destroyed after they return: every
  // worker drains its streams before returning, so no copy outlives the span.
  const std::unique_ptr<AutoPin> autopin = pin_on_the_fly(job, n);
  if (autopin) {
    job.src.pinned = job.src.autopinned = true;
    job.src.pin_lo = autopin->lo();
    job.src.pin_hi = autopin->hi();
  }
  if (const uint64_t hold = env_u64("LBF_TEST_AUTOPIN_HOLD_MS", 0); hold && autopin)
    std::this_thread::sleep_for(std::chrono::milliseconds(hold));  // tests only: keep the span pinned a while
  const size_t nw = ctx->workers.size();
  if (nw == 1 || n < 2 * nw) return worker_run(ctx->workers[0], job, 0, n);
  std::vector<int> rcs(nw, LBF_OK);
  std::vector<std::string> errs(nw);
  std::vector<std::thread> th;
  auto part = [&](size_t d, bool bind) {
    if (bind) bind_thread(ctx->workers[d].cpus);
    rcs[d] = guarded([&] { return worker_run(ctx->workers[d], job, n * d / nw, n * (d + 1) / nw); });
    if (rcs[d]) errs[d] = lbf_last_error();
  };
  std::vector<size_t> inline_parts;  // workers whose thread could not be started run here, in turn
  for (size_t d = 0; d < nw; ++d) {
    try {
      th.emplace_back(part, d, true);
    } catch (const std::system_error&) {
      inline_parts.push_back(d);
    }
  }
  for (size_t d : inline_parts) part(d, false);
  for (auto& t : th) t.join();
  for (size_t d = 0; d < nw; ++d)
    if (rcs[d])
      return fail(rcs[d], "worker " + std::to_string(d) + " (device " + std::to_string(ctx->workers[d].device) +
                              "): " + errs[d]);
  return LBF_OK;
}

int run_device_job(lbf_ctx* ctx, const uint8_t* base, const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                   uint8_t* digests, const uint8_t* expected, uint8_t* verdicts) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  KeepCurrentDevice keep;
  Worker& w = ctx->workers[0];
  LBF_HIP_TRY(hipSetDevice(w.device));
  hipStream_t s = w.dev[0].stream;
  for (uint64_t i = 0; i < n; i += 0xFFFFFFFFull) {
    const uint64_t cnt = std::min<uint64_t>(n - i, 0xFFFFFFFFull);
    int rc = lbf_sha1_launch(base, offsets + i, sizes + i, cnt, digests ? digests + 20 * i : nullptr,
                             expected ? expected + 20 * i : nullptr, verdicts ? verdicts + i : nullptr, s);
    if (rc) return rc;
  }
  LBF_HIP_TRY(hipStreamSynchronize(s));
  return LBF_OK;
}

}  // namespace lbf
