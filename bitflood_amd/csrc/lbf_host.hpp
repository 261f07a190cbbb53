// lbf_host.hpp -- what the host-side units of liblbfhash.so share (not part
// of the ABI): placement.cpp, staging.cpp, pinning.cpp, wire_batch.cpp and
// lbf_capi.cpp.
#pragma once

#include <stdint.h>

#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <system_error>
#include <vector>

#include "lbf_internal.hpp"
#include "stage_plan.hpp"

namespace lbf {

// Nothing is thrown across the C ABI: a host allocation that
// fails, or a thread that cannot be started, inside a call becomes a status.
template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(LBF_ERR_NOMEM, "host allocation failed");
  } catch (const std::system_error& e) {
    return fail(LBF_ERR_NOMEM, std::string("host resources: ") + e.what());
  } catch (const std::exception& e) {
    return fail(LBF_ERR_INVALID, std::string("internal error: ") + e.what());
  }
}

// ---- placement.cpp ----------------------------------------------------------
uint64_t env_u64(const char* name, uint64_t dflt);
long env_long(const char* name, long dflt);

// The caller's current HIP device is its own state (a torch process keeps its
// tensors on it): entry points that switch devices to create, drive or free
// workers put it back on the way out.
struct KeepCurrentDevice {
  int saved = -1;
  KeepCurrentDevice();
  ~KeepCurrentDevice();
};

bool numa_enabled();
int device_numa_node(int device);
std::vector<int> node_cpus_allowed(int node);  // the node's CPUs that this process may run on (empty: no binding)
void bind_thread(const std::vector<int>& cpus);
int page_node(const void* p);  // NUMA node of the page holding `p` (-1 when unknown)

// MPOL_PREFERRED(node) for the calling thread while in scope.
constexpr unsigned long kMaxNodes = 1024;
struct PreferNode {
  bool active = false;
  int old_mode = 0;
  unsigned long old_mask[kMaxNodes / 64] = {};
  explicit PreferNode(int node);
  ~PreferNode();
};

// Every exit of a synchronous entry point after its first async copy waits for
// the stream, so no copy is still reading a local staging vector or the
// caller's (possibly pinned) buffers, or writing into them, once the call has
// returned.  Declared after the host vectors the copies use, so it
// runs before they are destroyed.
struct SyncOnExit {
  hipStream_t st;
  ~SyncOnExit() {
    (void)hipStreamSynchronize(st);
    (void)hipGetLastError();
  }
};

// A call's device memory that a context keeps between calls (lbf_ctx::b64_dev,
// upd_dev): one allocation on the current device, replaced by one of `want`
// bytes when `need` does not fit; the caller holds ctx->mu and names itself in
// `who` for the message.
inline int grow_scratch(uint8_t*& dev, uint64_t& cap, uint64_t need, uint64_t want, const char* who) {
  if (need <= cap) return LBF_OK;
  if (dev) (void)hipFree(dev);
  dev = nullptr;
  cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(&dev), want) != hipSuccess) {
    (void)hipGetLastError();
    return fail(LBF_ERR_NOMEM, std::string(who) + ": device allocation of " + std::to_string(want) + " bytes");
  }
  cap = want;
  return LBF_OK;
}

// ---- staging.cpp ------------------------------------------------------------
// Staging is split in two rings.  A DEVICE slot in HBM holds one batch: the
// descriptors (offsets u64[cnt], sizes u32[cnt], expected 20 B x cnt, padded
// to kHdrAlign) and the chunk bytes, plus its stream and the batch's results;
// one kernel hashes the batch there and one D2H returns digests or verdicts.
// A HOST slot is a piece of pinned memory the batch's bytes pass through on
// their way to the device slot: a batch larger than a host slot is copied as
// several pieces (one H2D each) followed by its header, a batch that fits one
// host slot travels as one [header | data] copy.  A host slot is free again
// as soon as its H2D is done; a device slot only once its kernel is -- and
// that kernel lasts one chunk's serial SHA-1 chain (≈3.1 ms per 256 KiB of
// chunk, whatever the batch size).  So the device ring is sized per job to
// hold PCIe-rate x chain-time bytes in HBM (288 GB per GPU: the cheap place
// for bytes in flight), and the pinned ring stays small (LBF_SLOTS x
// LBF_PIN_MB): pinning is what a one-shot encode pays up front.
struct HostSlot {
  uint8_t* h_buf = nullptr;      // pinned, pin_bytes
  hipEvent_t copied = nullptr;   // recorded after the H2D that last read h_buf
  bool in_flight = false;
};

struct DevSlot {
  hipStream_t stream = nullptr;
  uint8_t* d_buf = nullptr;  // header | data (hdr_cap + slot_bytes)
  uint8_t* h_hdr = nullptr;  // pinned header of a multi-piece batch (hdr_cap)
  uint8_t* h_edge = nullptr;  // pinned bounce for a direct batch's bytes outside the pinned pages (edge_cap())
  uint8_t* d_out = nullptr;  // desc_cap * 20: digests, or verdicts
  uint8_t* h_out = nullptr;  // pinned
  std::vector<uint8_t> ok;   // 1 = chunk bytes fully available
  hipEvent_t copied = nullptr;  // recorded after a direct-route batch's last H2D (see stage_direct)
  // pending group (positions [g_begin, g_end)) to finalize after the stream drains
  bool pending = false;
  uint64_t g_begin = 0, g_end = 0;
};

class CopyPool;  // staging.cpp

struct Worker {
  int device = 0;
  int index = 0;            // position in the context
  int numa_node = -1;       // the device's NUMA node (-1: unknown / placement off)
  std::vector<int> cpus;    // CPUs its host threads bind to (empty: unbound)
  std::vector<HostSlot> host;  // LBF_SLOTS of them (default 3), used round-robin
  std::vector<DevSlot> dev;    // at least as many; grown per job for long chains, trimmed after it
  uint64_t slot_bytes = 0;  // current data capacity per device slot (grown on demand)
  uint64_t slot_max = 0;    // LBF_SLOT_MB: the largest a device slot may grow
  uint64_t pin_bytes = 0;   // current size of each pinned host slot (grown on demand)
  uint64_t pin_max = 0;     // LBF_PIN_MB: the largest a host slot may grow
  uint64_t dev_budget = 0;  // LBF_DEVICE_STAGING_MB: HBM for device slots
  uint64_t desc_cap = 0;    // descriptors per group
  uint64_t hdr_cap = 0;     // header_bytes(desc_cap)
  uint64_t bytes_staged = 0;  // chunk bytes sent through the pinned ring (cumulative)
  uint64_t bytes_direct = 0;  // chunk bytes sent straight from registered caller memory
  long fault_group = -1;    // LBF_TEST_FAULT_GROUP (tests only, one shot)
  bool fault_throws = false;  // LBF_TEST_FAULT_KIND=throw: the fault is a host exception, not a HIP error
  std::shared_ptr<CopyPool> pool;  // staging copy helpers, started by the first job that needs them (one owner)
};

int worker_init(Worker& w, int device, int index);
void worker_free(Worker& w);

// Host threads per staging copy: LBF_COPY_THREADS, default 8 (a GPU box's
// share of host cores is 16; two devices' workers may copy at once).
unsigned copy_threads();

// Where a job's bytes come from: caller memory (bounds-checked up front) or
// files read with pread (one descriptor table over several files: each
// descriptor names its file).  read_serial() returns the bytes available.
struct Source {
  const uint8_t* base = nullptr;  // memory source
  uint64_t base_len = 0;
  std::vector<int> fds;           // file source: one fd per file, -1 = could not be opened
  bool pinned = false;            // [base, base+base_len) lies in a lbf_host_register'ed range
  bool autopinned = false;        // ... or in the span run_job pinned for this job (pin_on_the_fly)
  // The pinned addresses of a pinned source, [pin_lo, pin_hi): all of it for
  // a registered one; for an on-the-fly one the pages wholly inside the job's
  // bytes, so up to a page at either end lies outside (bounced, stage_direct).
  uintptr_t pin_lo = 0, pin_hi = 0;
  unsigned threads = copy_threads();  // staging copy threads

  bool from_files() const { return !fds.empty(); }
  bool exists(uint32_t file) const { return !from_files() || fds[file] >= 0; }
  uint64_t read_serial(uint8_t* dst, uint32_t file, uint64_t off, uint64_t len) const;
};

struct Job : Table {
  Source src;
  const uint8_t* expected = nullptr;  // null => hash mode
  uint8_t* digests = nullptr;         // hash mode output
  uint8_t* verdicts = nullptr;        // verify mode output
};

int run_job(lbf_ctx* ctx, Job job, uint64_t n);
// Device-pointer batch: synchronous on worker 0's first stream.
int run_device_job(lbf_ctx* ctx, const uint8_t* base, const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                   uint8_t* digests, const uint8_t* expected, uint8_t* verdicts);

// ---- pinning.cpp ------------------------------------------------------------
// Caller memory registered with lbf_host_register: [lo, hi) page-rounded, as
// pinned; `owned` = this context registered it (and unregisters it).
struct Registered {
  uintptr_t user = 0;  // the pointer the caller passed (the unregister key)
  uintptr_t user_end = 0;  // user + the length the caller passed
  uintptr_t lo = 0, hi = 0;
  bool owned = false;
};

// A memory source lies in a registered range of the context.
bool in_registered(const lbf_ctx* ctx, const uint8_t* base, uint64_t len);
int host_register(lbf_ctx* ctx, const void* ptr, uint64_t len);
int host_unregister(lbf_ctx* ctx, const void* ptr);
int unpin(uintptr_t lo);  // drop one reference to the pin at lo (pinned by this library)

// The pages wholly inside a job's bytes, registered for the life of the
// object (see pinning.cpp).
class AutoPin {
 public:
  AutoPin(uintptr_t lo, uintptr_t hi);
  ~AutoPin();
  AutoPin(const AutoPin&) = delete;
  AutoPin& operator=(const AutoPin&) = delete;
  bool pinned() const { return pinned_; }
  uintptr_t lo() const { return lo_; }
  uintptr_t hi() const { return hi_; }

 private:
  uintptr_t lo_ = 0, hi_ = 0;
  bool reserved_ = false, pinned_ = false;
};
std::unique_ptr<AutoPin> pin_on_the_fly(const Job& job, uint64_t n);

}  // namespace lbf

struct lbf_ctx {
  std::vector<lbf::Worker> workers;
  std::vector<lbf::Registered> regs;  // guarded by mu, like every job
  // lbf_b64_verify_batch's device memory (text, sextets, bytes, tables) on
  // worker 0's device: one allocation, grown on demand, guarded by mu
  uint8_t* b64_dev = nullptr;
  uint64_t b64_cap = 0;
  // lbf_b64_verify_batch's chunks by decode path (lbf_ctx_b64_stats), guarded by mu
  uint64_t b64_one_pass = 0, b64_general = 0;
  // lbf_sha1_update_batch's device memory (bytes, states, tables) on worker 0's
  // device, grown on demand, guarded by mu; and the piece bytes one of its
  // launches may carry (LBF_UPDATE_MB, read at creation)
  uint8_t* upd_dev = nullptr;
  uint64_t upd_cap = 0;
  uint64_t update_bytes = 256ull << 20;
  // lbf_b64_update_batch's characters by decode path (lbf_ctx_b64_update_stats), guarded by mu
  uint64_t b64_line_chars = 0, b64_scan_chars = 0;
  // the flat path's share of the two above (lbf_ctx_b64_flat_stats), guarded by mu: b64_general's chunks the
  // flat pass decoded, b64_scan_chars' characters the flat kernel took
  uint64_t b64_flat_chunks = 0, b64_flat_chars = 0;
  mutable std::mutex mu;
};
