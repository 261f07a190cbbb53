// pinning.cpp -- caller memory the device reads without a staging copy: the
// process-wide pin table behind lbf_host_register, and the pages a job pins on
// the fly (LBF_AUTOPIN=1).
//
// Caller-pinned sources (lbf_host_register).  hipHostRegister pins whole
// pages, portably (every device can DMA from them).  HIP does not count
// registrations per caller: when a second context registered and then
// unregistered a range the first one held, the first one's pin was gone
// (its hipHostUnregister then failed; tests/test_gpu_registered.py, first
// run).  So the library keeps one process-wide pin table: contexts
// registering the same range share one pin (reference-counted), and memory
// that something else already pinned (a hipHostMalloc'd buffer, a caller's
// own hipHostRegister) is used as it is and never unpinned here.
//
// Pinning a large pageable job on the fly (opt-in with
// LBF_AUTOPIN=1: on by default in round 5, off since round 6).  A pageable job
// crosses host DRAM three times on the staged route (the caller's write, the
// staging memcpy's read and write, the DMA's read); a registered one once (§3).
// Round 5 timed hipHostRegister of a 4 GiB span at ~0.1 ms and turned this on,
// but that span had been registered before in the same process: on pages
// registered for the first time it costs 168-233 ms per 4 GiB of touched 4 KiB
// pages (the kind new[]/malloc give; 7.5 ms on transparent huge pages, ~700 ms
// on pages never touched), and only re-registering pages HIP has seen is cheap
// (tools/register_cost.py, profiles/r06/register_cost/).  So a job on a fresh
// 4 KiB-page buffer ran 3.6x slower pinned than staged at 4 GiB (294 against
// 81 ms) and 3.4x at 1 GiB, while a warm one gained 0-8 %.  A caller that hashes
// one buffer repeatedly registers it once (lbf_host_register); LBF_AUTOPIN=1
// pins each large job's pages for the job.  When on, run_job registers them in
// one piece before any worker starts and unregisters after every worker has
// drained; the workers see a registered source and take the direct route.  One
// registration per JOB, not per worker: the workers' index ranges meet inside
// a page unless the buffer is page-aligned, and two registrations of one page
// are refused below (round 5 first pinned per worker, and with two workers one
// of them staged).  A span HIP refuses to register is staged, and so is a
// batch whose copy HIP refuses (staging.cpp, stage_direct).
//
// The pages pinned on the fly by running jobs are kept process-wide, [lo, hi)
// each.  Two contexts hashing the same pageable buffer at once must not both
// register it (one's unregister could drop pages the other is still copying
// from), so a span that overlaps another job's, or a range pinned through
// lbf_host_register, is staged.  The other direction matters as much (ADVICE
// r05): lbf_host_register must never take a job's pages for "pinned by
// someone else" and adopt them, since the job unpins them when it ends; it
// waits on g_autopin_cv until no running job's pages overlap its range.  Lock
// order: a context's mu, then g_autopin_mu, then g_pin_mu.
#include <hip/hip_runtime.h>
#include <hsa/hsa_ext_amd.h>
#include <unistd.h>

#include <condition_variable>
#include <iterator>
#include <map>

#include "lbf_host.hpp"

namespace lbf {

namespace {

struct Pin {
  uintptr_t hi = 0;
  uint64_t refs = 0;
};
using PinMap = std::map<uintptr_t, Pin>;  // lo -> pin, disjoint ranges

// [lo, hi) overlaps a range of the map.
bool overlaps(const PinMap& m, uintptr_t lo, uintptr_t hi) {
  auto next = m.lower_bound(lo);
  return (next != m.end() && next->first < hi) || (next != m.begin() && std::prev(next)->second.hi > lo);
}

std::mutex g_pin_mu;
PinMap g_pins;

std::mutex g_autopin_mu;
std::condition_variable g_autopin_cv;       // notified when a span is released
PinMap g_autopin;                     // the spans reserved now (one reference each)

bool reserve_autopin(uintptr_t lo, uintptr_t hi) {
  std::lock_guard<std::mutex> g(g_autopin_mu);
  if (overlaps(g_autopin, lo, hi)) return false;
  {
    std::lock_guard<std::mutex> pins(g_pin_mu);
    if (overlaps(g_pins, lo, hi)) return false;
  }
  g_autopin[lo] = Pin{hi, 1};
  return true;
}

void release_autopin(uintptr_t lo) {
  {
    std::lock_guard<std::mutex> g(g_autopin_mu);
    g_autopin.erase(lo);
  }
  g_autopin_cv.notify_all();
}

}  // namespace

// The pages wholly inside the job's bytes [lo, hi), registered for the life of
// the object (the owner destroys it only once every copy from them has
// landed).  Rounding inward, not outward, is what keeps the library off memory
// it was not handed: the first and last page of a span
// that does not start and end on a page boundary also hold the caller's other
// data, which the caller may pin itself while the job runs (an outward span
// made that hipHostRegister fail), so they stay pageable and a direct batch
// bounces the few bytes of the job that lie on them (staging.cpp, DirectCopies).
AutoPin::AutoPin(uintptr_t lo, uintptr_t hi) {
  const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE);
  lo_ = (lo + page - 1) & ~(page - 1);
  hi_ = hi & ~(page - 1);
  if (lo_ >= hi_ || !reserve_autopin(lo_, hi_)) return;  // another job pins (part of) it, or the caller does: staged
  reserved_ = true;
  const hipError_t e = hipHostRegister(reinterpret_cast<void*>(lo_), hi_ - lo_, hipHostRegisterPortable);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // pinned elsewhere, or no memory: the job is staged
    return;
  }
  pinned_ = true;
}

AutoPin::~AutoPin() {
  if (pinned_) {
    (void)hipHostUnregister(reinterpret_cast<void*>(lo_));
    (void)hipGetLastError();
  }
  if (reserved_) release_autopin(lo_);
}

// The registration run_job makes for a memory job of LBF_AUTOPIN_MIN_MB (64)
// and more whose chunks cover their address span without a gap
// (stage_plan.hpp, gap_free_cover), or null.  A table with gaps is staged:
// pinning across a gap pins pages no copy reads, bytes the caller did not hand
// over (round 5 pinned any span its chunks filled half of).  A span larger
// than half of the host's physical memory is staged too: pinning it would lock
// most of RAM for the length of the call.
std::unique_ptr<AutoPin> pin_on_the_fly(const Job& job, uint64_t n) {
  if (job.src.from_files() || job.src.pinned || env_long("LBF_AUTOPIN", 0) != 1) return nullptr;
  const uint64_t min_bytes = env_u64("LBF_AUTOPIN_MIN_MB", 64) << 20;
  uint64_t lo = 0, hi = 0;
  if (!gap_free_cover(job.offsets, job.sizes, n, min_bytes, lo, hi)) return nullptr;
  const long pages = sysconf(_SC_PHYS_PAGES), page = sysconf(_SC_PAGESIZE);
  if (pages > 0 && page > 0 && hi - lo > (uint64_t)pages * (uint64_t)page / 2) return nullptr;
  const uintptr_t b = reinterpret_cast<uintptr_t>(job.src.base);
  std::unique_ptr<AutoPin> pin(new AutoPin(b + lo, b + hi));
  if (!pin->pinned()) pin.reset();
  return pin;
}

// A memory source lies in a registered range: the pages this library pinned,
// or, for memory pinned by someone else, the caller's own bytes (only those
// were shown to lie in one pinned allocation, host_register).
bool in_registered(const lbf_ctx* ctx, const uint8_t* base, uint64_t len) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(base);
  for (const Registered& r : ctx->regs) {
    const uintptr_t lo = r.owned ? r.lo : r.user, hi = r.owned ? r.hi : r.user_end;
    if (a >= lo && a <= hi && len <= hi - a) return true;
  }
  return false;
}

namespace {

// The pinned host allocation that holds address p, as [base, end), if any.
// hipMemGetAddressRange resolves host-pinned memory (hipHostMalloc,
// hipHostRegister) by the host address or, failing that, by the device
// address hipPointerGetAttributes reports for it.
struct PinnedAlloc {
  bool pinned = false;
  uintptr_t base = 0, end = 0;  // end == 0: the extent is unknown
  uint64_t id = 0;              // HIP's buffer id of the allocation (0: unknown)
};
PinnedAlloc pinned_alloc(uintptr_t p) {
  PinnedAlloc out;
  // The runtime under HIP reports the host base and size of the allocation a
  // pinned pointer lies in, for hipHostMalloc (an HSA pool allocation) and for
  // hipHostRegister (locked) memory alike.  hipMemGetAddressRange gives the
  // size of a hipHostRegister'd range but a null base (measured on the box,
  // tools/pin_extent_probe.py), so it is only the fallback.
  hsa_amd_pointer_info_t info{};
  info.size = sizeof(info);
  if (hsa_amd_pointer_info(reinterpret_cast<const void*>(p), &info, nullptr, nullptr, nullptr) == HSA_STATUS_SUCCESS &&
      (info.type == HSA_EXT_POINTER_TYPE_LOCKED || info.type == HSA_EXT_POINTER_TYPE_HSA) && info.hostBaseAddress &&
      info.sizeInBytes) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(info.hostBaseAddress);
    if (b <= p && p - b < info.sizeInBytes) {
      out.pinned = true;
      out.base = b;
      out.end = b + info.sizeInBytes;
      return out;
    }
  }
  hipPointerAttribute_t attr{};
  out.pinned = hipPointerGetAttributes(&attr, reinterpret_cast<void*>(p)) == hipSuccess &&
               attr.type == hipMemoryTypeHost;
  (void)hipGetLastError();  // pageable memory is an error to that query
  if (!out.pinned) return out;
  // One id per allocation or registration: two addresses with the same id lie
  // in one allocation, and so does every byte between them.
  unsigned long long id = 0;
  if (hipPointerGetAttribute(&id, HIP_POINTER_ATTRIBUTE_BUFFER_ID, reinterpret_cast<hipDeviceptr_t>(p)) == hipSuccess)
    out.id = id;
  (void)hipGetLastError();
  const uintptr_t dev = reinterpret_cast<uintptr_t>(attr.devicePointer);
  for (const uintptr_t q : {p, dev}) {
    hipDeviceptr_t b = nullptr;
    size_t size = 0;
    const bool ok = q && hipMemGetAddressRange(&b, &size, reinterpret_cast<hipDeviceptr_t>(q)) == hipSuccess;
    (void)hipGetLastError();
    const uintptr_t bb = reinterpret_cast<uintptr_t>(b);
    if (ok && size && bb <= q && q - bb < size) {
      out.base = p - (q - bb);  // the same offset from the host base
      out.end = out.base + size;
      return out;
    }
  }
  return out;
}

// Pin the page-rounded range of r, or adopt it: the caller holds ctx->mu,
// g_autopin_mu and g_pin_mu, and no entry of g_pins overlaps the range.
int pin_or_adopt(lbf_ctx* ctx, Registered& r) {
  // Pinned already by someone else (a hipHostMalloc'd buffer, a caller's own
  // registration): use it, never unpin it -- but only if ONE pinned
  // allocation covers the caller's whole range.  Its first and last byte
  // being pinned is not enough: they may belong to two neighbouring
  // allocations with pageable memory between them, which a direct copy would
  // then read.  The caller's bytes [user, user_end) are what is checked (a
  // buffer pinned whole by the caller need not end on a page boundary).
  const uintptr_t a = r.user, uend = r.user_end;
  const PinnedAlloc first = pinned_alloc(a), last = pinned_alloc(uend - 1);
  if ((first.pinned && first.end && first.base <= a && uend <= first.end) ||
      (first.pinned && last.pinned && first.id && first.id == last.id))
    return LBF_OK;
  if (first.pinned && !first.end && !first.id)
    return fail(LBF_ERR_INVALID,
                "lbf_host_register: range is pinned already, but HIP does not report the extent of the pinned "
                "allocation holding it, so it cannot be shown to cover the range");
  if (first.pinned || last.pinned)
    return fail(LBF_ERR_INVALID,
                "lbf_host_register: range is partly pinned already (no single pinned allocation holds all of it)");
  KeepCurrentDevice keep;
  LBF_HIP_TRY(hipSetDevice(ctx->workers[0].device));
  const hipError_t e = hipHostRegister(reinterpret_cast<void*>(r.lo), r.hi - r.lo, hipHostRegisterPortable);
  if (e == hipErrorHostMemoryAlreadyRegistered) {
    // pages inside the range are pinned by another allocation while its
    // first and last are not (checked above): partly pinned
    (void)hipGetLastError();
    return fail(LBF_ERR_INVALID, "lbf_host_register: range is partly pinned already (pages inside it belong to "
                                 "another pinned allocation)");
  }
  if (e != hipSuccess) return hip_fail(e, "hipHostRegister");
  g_pins[r.lo] = Pin{r.hi, 1};
  r.owned = true;
  return LBF_OK;
}

}  // namespace

int unpin(uintptr_t lo) {
  std::lock_guard<std::mutex> lock(g_pin_mu);
  auto it = g_pins.find(lo);
  if (it == g_pins.end()) return LBF_OK;
  if (--it->second.refs) return LBF_OK;
  g_pins.erase(it);
  LBF_HIP_TRY(hipHostUnregister(reinterpret_cast<void*>(lo)));
  return LBF_OK;
}

int host_register(lbf_ctx* ctx, const void* ptr, uint64_t len) {
  const uintptr_t page = (uintptr_t)sysconf(_SC_PAGESIZE);
  const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
  if (len > UINTPTR_MAX - a - page) return fail(LBF_ERR_INVALID, "lbf_host_register: range wraps");
  Registered r;
  r.user = a;
  r.user_end = a + len;
  r.lo = a & ~(page - 1);
  r.hi = (a + len + page - 1) & ~(page - 1);
  return guarded([&] {
    std::lock_guard<std::mutex> lock(ctx->mu);
    for (const Registered& o : ctx->regs)
      if (r.lo < o.hi && o.lo < r.hi)
        return fail(LBF_ERR_INVALID,
                    "lbf_host_register: range shares pages with one this context already holds (pinning is per "
                    "page: give each registered buffer pages of its own)");
    ctx->regs.reserve(ctx->regs.size() + 1);  // nothing below may throw once pinned
    // Pages a running job pinned on the fly are that job's: it unpins them
    // when it ends.  Taken below for "pinned by someone else", they would
    // leave this registration pointing at pageable memory and its batches
    // copying "directly" from it.  So wait for every such job to
    // end; holding g_autopin_mu from here on keeps a new job from pinning the
    // range before it is in g_pins (reserve_autopin checks that table).
    std::unique_lock<std::mutex> spans(g_autopin_mu);
    g_autopin_cv.wait(spans, [&] { return !overlaps(g_autopin, r.lo, r.hi); });
    std::lock_guard<std::mutex> pins(g_pin_mu);
    auto same = g_pins.find(r.lo);
    if (same != g_pins.end() && same->second.hi == r.hi) {
      ++same->second.refs;  // the same range, pinned by another context
      r.owned = true;
    } else if (overlaps(g_pins, r.lo, r.hi)) {
      return fail(LBF_ERR_INVALID, "lbf_host_register: range overlaps, but differs from, one another context holds");
    } else if (int rc = pin_or_adopt(ctx, r)) {
      return rc;
    }
    ctx->regs.push_back(r);
    return (int)LBF_OK;
  });
}

int host_unregister(lbf_ctx* ctx, const void* ptr) {
  std::lock_guard<std::mutex> lock(ctx->mu);  // no job is reading it
  const uintptr_t a = reinterpret_cast<uintptr_t>(ptr);
  for (size_t k = 0; k < ctx->regs.size(); ++k) {
    if (ctx->regs[k].user != a) continue;
    const Registered r = ctx->regs[k];
    ctx->regs.erase(ctx->regs.begin() + (long)k);
    return r.owned ? unpin(r.lo) : LBF_OK;
  }
  return fail(LBF_ERR_INVALID, "lbf_host_unregister: pointer was not registered with this context");
}

}  // namespace lbf
