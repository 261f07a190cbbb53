// lbf_capi.cpp -- the C ABI of liblbfhash.so: error slot, base64-27, device
// and stream helpers, the lbf_ctx's life and numbers, and the memory and file
// entry points.
//
// The context is the batched replacement for the reference's per-chunk
// fread -> Base64Encode loop (Encoder.cpp:54-72) and the per-chunk verify
// loops (Flood.cpp:246-285, ChunkMethods.cpp:111-128, 156-167): the caller
// hands over a descriptor table, the context copies the covered byte ranges
// into device slots (staging.cpp; LBF_SLOTS of them, round-robin: host memcpy
// of group g+1 overlaps H2D + kernel + D2H of the groups before it) and
// returns digests or verdicts.
// Multiple devices take contiguous index ranges, one host thread each, with no
// collective.  Placement is in placement.cpp, registered and
// on-the-fly pinned sources in pinning.cpp, the wire (base64) batch calls in
// wire_batch.cpp.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <string.h>
#include <sys/resource.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>

#include "lbf_host.hpp"

namespace lbf {

namespace {
thread_local std::string t_last_error;
}

void set_error(const std::string& msg) { t_last_error = msg; }
const char* last_error_cstr() { return t_last_error.c_str(); }

int fail(int status, const std::string& msg) {
  set_error(msg);
  return status;
}

int hip_fail(hipError_t e, const char* what) {
  // HIP keeps a failed call's status as the thread's last error; left there,
  // it surfaces from the hipGetLastError() after the NEXT kernel launch and
  // fails a call that did nothing wrong.  The status is reported here instead.
  (void)hipGetLastError();
  return fail(e == hipErrorOutOfMemory ? LBF_ERR_NOMEM : LBF_ERR_HIP,
              std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace lbf

using namespace lbf;

// ---------------------------------------------------------------------------
// base64-27 (BaseN_Encoder(alphabet, 6), no padding: basecode.cpp:13-37,39-104;
// alphabet Encoder.cpp:104-105).  20 bytes = 160 bits = 26 full sextets plus
// one 4-bit tail sextet, MSB first, zero-filled on the right.
// ---------------------------------------------------------------------------
static const char kAlphabet[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";

extern "C" void lbf_b64_27(const uint8_t digest[20], char out[28]) {
  int o = 0;
  // 6 groups of 3 bytes -> 24 chars, then 2 bytes -> 3 chars (last one partial)
  for (int g = 0; g < 6; ++g) {
    const uint32_t v = (uint32_t(digest[3 * g]) << 16) | (uint32_t(digest[3 * g + 1]) << 8) | digest[3 * g + 2];
    out[o++] = kAlphabet[(v >> 18) & 63];
    out[o++] = kAlphabet[(v >> 12) & 63];
    out[o++] = kAlphabet[(v >> 6) & 63];
    out[o++] = kAlphabet[v & 63];
  }
  const uint32_t v = (uint32_t(digest[18]) << 8) | digest[19];  // 16 bits
  out[o++] = kAlphabet[(v >> 10) & 63];
  out[o++] = kAlphabet[(v >> 4) & 63];
  out[o++] = kAlphabet[(v << 2) & 63];
  out[o] = '\0';
}

static int b64_value(char c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}

extern "C" int lbf_b64_27_decode(const char* in, size_t len, uint8_t out[20]) {
  if (!in || !out || len != 27) return fail(LBF_ERR_INVALID, "b64_27_decode: need exactly 27 chars");
  uint32_t acc = 0;
  int bits = 0, o = 0;
  for (size_t i = 0; i < 27; ++i) {
    const int v = b64_value(in[i]);
    if (v < 0) return fail(LBF_ERR_INVALID, "b64_27_decode: character outside the alphabet");
    acc = (acc << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      if (o < 20) out[o++] = (uint8_t)(acc >> bits);
      acc &= (1u << bits) - 1u;
    }
  }
  // 162 bits read, 160 used: the 2 leftover bits must be zero (canonical form)
  if (o != 20 || bits != 2 || acc != 0) return fail(LBF_ERR_INVALID, "b64_27_decode: non-canonical tail");
  return LBF_OK;
}

// ---------------------------------------------------------------------------
// Library / device helpers
// ---------------------------------------------------------------------------
extern "C" int lbf_abi_version(void) { return LBF_ABI_VERSION; }

extern "C" const char* lbf_last_error(void) { return lbf::last_error_cstr(); }

extern "C" int lbf_device_count(int* out) {
  if (!out) return fail(LBF_ERR_INVALID, "null out");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *out = n;
  return LBF_OK;
}

extern "C" int lbf_dev_malloc(void** out, uint64_t bytes) {
  if (!out) return fail(LBF_ERR_INVALID, "null out");
  LBF_HIP_TRY(hipMalloc(out, bytes ? bytes : 1));
  return LBF_OK;
}
extern "C" int lbf_dev_free(void* p) {
  LBF_HIP_TRY(hipFree(p));
  return LBF_OK;
}
extern "C" int lbf_memcpy_h2d(void* dst, const void* src, uint64_t bytes) {
  LBF_HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return LBF_OK;
}
extern "C" int lbf_memcpy_d2h(void* dst, const void* src, uint64_t bytes) {
  LBF_HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return LBF_OK;
}
extern "C" int lbf_set_device(int d) {
  LBF_HIP_TRY(hipSetDevice(d));
  return LBF_OK;
}
extern "C" int lbf_device_synchronize(void) {
  LBF_HIP_TRY(hipDeviceSynchronize());
  return LBF_OK;
}
extern "C" int lbf_stream_create(void** out) {
  if (!out) return fail(LBF_ERR_INVALID, "null out");
  hipStream_t s;
  LBF_HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *out = (void*)s;
  return LBF_OK;
}
extern "C" int lbf_stream_destroy(void* s) {
  LBF_HIP_TRY(hipStreamDestroy((hipStream_t)s));
  return LBF_OK;
}
extern "C" int lbf_stream_synchronize(void* s) {
  LBF_HIP_TRY(hipStreamSynchronize((hipStream_t)s));
  return LBF_OK;
}

// ---------------------------------------------------------------------------
// Context: workers (one per device, or LBF_WORKERS_PER_DEVICE per device for
// tests) with LBF_SLOTS pipeline slots each.
// ---------------------------------------------------------------------------
extern "C" int lbf_ctx_create(uint32_t device_mask, lbf_ctx** out) {
  if (!out) return fail(LBF_ERR_INVALID, "null out");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(LBF_ERR_NO_DEVICE, "no GPU visible: the chunk-hash path runs only on MI355X (no CPU fallback)");
  // Test knob: k workers per selected device, so the multi-worker split, the
  // per-worker staging and the error propagation of run_job run on a one-GPU
  // box exactly as they do with one worker per GPU on an 8-GPU node.
  const int per_dev = (int)std::max(1L, std::min(16L, env_long("LBF_WORKERS_PER_DEVICE", 1)));
  KeepCurrentDevice keep;  // worker_init selects each worker's device
  lbf_ctx* ctx = new (std::nothrow) lbf_ctx();
  if (!ctx) return fail(LBF_ERR_NOMEM, "host allocation failed");
  // piece bytes per launch of lbf_sha1_update_batch: 1 MiB .. 64 GiB
  ctx->update_bytes = std::max<uint64_t>(1, std::min<uint64_t>(65536, env_u64("LBF_UPDATE_MB", 256))) << 20;
  const int rc = guarded([&] {
    ctx->workers.reserve((size_t)std::min(ndev, 32) * (size_t)per_dev);  // workers never move once initialised
    for (int d = 0; d < ndev && d < 32; ++d) {
      if (device_mask && !(device_mask & (1u << d))) continue;
      for (int k = 0; k < per_dev; ++k) {
        ctx->workers.emplace_back();
        if (int r = worker_init(ctx->workers.back(), d, (int)ctx->workers.size() - 1)) return r;
      }
    }
    return (int)LBF_OK;
  });
  if (rc) {
    std::string msg = lbf_last_error();
    lbf_ctx_destroy(ctx);
    return fail(rc, msg);
  }
  if (ctx->workers.empty()) {
    delete ctx;
    return fail(LBF_ERR_NO_DEVICE, "device_mask selects no visible device");
  }
  *out = ctx;
  return LBF_OK;
}

extern "C" int lbf_ctx_worker_info(const lbf_ctx* ctx, int worker, int* device, int* numa_node, int* staging_node,
                                   int* bound_cpus) {
  if (!ctx || worker < 0 || worker >= (int)ctx->workers.size()) return fail(LBF_ERR_INVALID, "no such worker");
  // a running job may grow or trim the slots read below: wait for it
  std::lock_guard<std::mutex> lock(ctx->mu);
  const Worker& w = ctx->workers[worker];
  if (device) *device = w.device;
  if (numa_node) *numa_node = w.numa_node;
  if (staging_node)
    *staging_node = page_node(!w.host.empty() && w.host[0].h_buf ? (const void*)w.host[0].h_buf
                                                                 : (w.dev.empty() ? nullptr : (const void*)w.dev[0].h_out));
  if (bound_cpus) *bound_cpus = (int)w.cpus.size();
  return LBF_OK;
}

extern "C" void lbf_ctx_destroy(lbf_ctx* ctx) {
  if (!ctx) return;
  KeepCurrentDevice keep;
  if ((ctx->b64_dev || ctx->upd_dev) && !ctx->workers.empty() && hipSetDevice(ctx->workers[0].device) == hipSuccess) {
    if (ctx->b64_dev) (void)hipFree(ctx->b64_dev);
    if (ctx->upd_dev) (void)hipFree(ctx->upd_dev);
  }
  for (Worker& w : ctx->workers) worker_free(w);
  for (const Registered& r : ctx->regs)
    if (r.owned) (void)unpin(r.lo);  // teardown: nowhere to report a failure
  delete ctx;
}

extern "C" int lbf_ctx_num_devices(const lbf_ctx* ctx) {
  if (!ctx) return 0;
  int n = 0;
  for (size_t k = 0; k < ctx->workers.size(); ++k) n += (k == 0 || ctx->workers[k].device != ctx->workers[k - 1].device);
  return n;
}

extern "C" int lbf_ctx_num_workers(const lbf_ctx* ctx) { return ctx ? (int)ctx->workers.size() : 0; }

extern "C" int lbf_ctx_b64_stats(lbf_ctx* ctx, uint64_t* one_pass_chunks, uint64_t* general_chunks) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (one_pass_chunks) *one_pass_chunks = ctx->b64_one_pass;
  if (general_chunks) *general_chunks = ctx->b64_general;
  return LBF_OK;
}

extern "C" int lbf_ctx_b64_update_stats(lbf_ctx* ctx, uint64_t* line_chars, uint64_t* scan_chars) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (line_chars) *line_chars = ctx->b64_line_chars;
  if (scan_chars) *scan_chars = ctx->b64_scan_chars;
  return LBF_OK;
}

extern "C" int lbf_ctx_b64_flat_stats(lbf_ctx* ctx, uint64_t* flat_chunks, uint64_t* flat_chars) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (flat_chunks) *flat_chunks = ctx->b64_flat_chunks;
  if (flat_chars) *flat_chars = ctx->b64_flat_chars;
  return LBF_OK;
}

extern "C" int lbf_ctx_staging_stats(lbf_ctx* ctx, uint64_t* staged_bytes, uint64_t* direct_bytes) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  std::lock_guard<std::mutex> lock(ctx->mu);  // between jobs
  uint64_t st = 0, di = 0;
  for (const Worker& w : ctx->workers) st += w.bytes_staged, di += w.bytes_direct;
  if (staged_bytes) *staged_bytes = st;
  if (direct_bytes) *direct_bytes = di;
  return LBF_OK;
}

// Caller-pinned sources: see the pin table in pinning.cpp.
extern "C" int lbf_host_register(lbf_ctx* ctx, const void* ptr, uint64_t len) {
  if (!ctx || !ptr || len == 0) return fail(LBF_ERR_INVALID, "lbf_host_register: null context/pointer or empty range");
  return host_register(ctx, ptr, len);
}

extern "C" int lbf_host_unregister(lbf_ctx* ctx, const void* ptr) {
  if (!ctx || !ptr) return fail(LBF_ERR_INVALID, "lbf_host_unregister: null context/pointer");
  return host_unregister(ctx, ptr);
}

namespace {

// A job over caller memory [base, base + base_len), every chunk inside it;
// the caller sets the outputs.
int memory_job(Job& job, const uint8_t* base, uint64_t base_len, const uint64_t* offsets, const uint32_t* sizes,
               uint64_t n) {
  job.src.base = base;
  job.src.base_len = base_len;
  job.offsets = offsets;
  job.sizes = sizes;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t o = offsets[i], sz = sizes[i];
    if (o > base_len || sz > base_len - o)
      return fail(LBF_ERR_INVALID, "chunk " + std::to_string(i) + " lies outside [base, base+base_len)");
  }
  return LBF_OK;
}

}  // namespace

extern "C" int lbf_sha1_batch(lbf_ctx* ctx, const uint8_t* base, uint64_t base_len, const uint64_t* offsets,
                              const uint32_t* sizes, uint64_t n, uint8_t* out_digests, int flags) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (!base || !offsets || !sizes || !out_digests) return fail(LBF_ERR_INVALID, "null argument");
  if (flags == LBF_DEVICE_PTR) return run_device_job(ctx, base, offsets, sizes, n, out_digests, nullptr, nullptr);
  if (flags != LBF_HOST_PTR) return fail(LBF_ERR_INVALID, "unknown flags");
  Job job{};
  job.digests = out_digests;
  if (int rc = memory_job(job, base, base_len, offsets, sizes, n)) return rc;
  return guarded([&] { return run_job(ctx, job, n); });
}

extern "C" int lbf_verify_batch(lbf_ctx* ctx, const uint8_t* base, uint64_t base_len, const uint64_t* offsets,
                                const uint32_t* sizes, uint64_t n, const uint8_t* expected, uint8_t* verdicts,
                                int flags) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (!base || !offsets || !sizes || !expected || !verdicts) return fail(LBF_ERR_INVALID, "null argument");
  if (flags == LBF_DEVICE_PTR) return run_device_job(ctx, base, offsets, sizes, n, nullptr, expected, verdicts);
  if (flags != LBF_HOST_PTR) return fail(LBF_ERR_INVALID, "unknown flags");
  Job job{};
  job.expected = expected;
  job.verdicts = verdicts;
  if (int rc = memory_job(job, base, base_len, offsets, sizes, n)) return rc;
  return guarded([&] { return run_job(ctx, job, n); });
}

namespace {

// Files one job holds open at once: a quarter of the soft RLIMIT_NOFILE, so a
// caller with sockets and other descriptors still has room (EncodeFile opens
// one file at a time in the reference, Encoder.cpp:40-79); LBF_FILES_WINDOW
// overrides.  A flood with more files runs as one job per window of files.
uint32_t files_window() {
  if (uint64_t w = env_u64("LBF_FILES_WINDOW", 0)) return (uint32_t)std::min<uint64_t>(w, 1u << 20);
  rlimit rl{};
  uint64_t soft = 1024;
  if (getrlimit(RLIMIT_NOFILE, &rl) == 0 && rl.rlim_cur != RLIM_INFINITY) soft = rl.rlim_cur;
  return (uint32_t)std::max<uint64_t>(4, std::min<uint64_t>(4096, soft / 4));
}

// One job over files [0, n_files) of `paths`, all opened up front.
int files_ranges_job(lbf_ctx* ctx, const char* const* paths, uint32_t n_files, const uint32_t* file_of,
                     const uint64_t* offsets, const uint32_t* sizes, uint64_t n, const uint8_t* expected,
                     uint8_t* out) {
  Job job{};
  job.src.fds.assign(n_files, -1);
  struct Closer {  // every opened file is closed on every path
    std::vector<int>& fds;
    ~Closer() {
      for (int fd : fds)
        if (fd >= 0) close(fd);
    }
  } closer{job.src.fds};
  for (uint32_t f = 0; f < n_files; ++f) {
    const int fd = open(paths[f], O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
      // Out of descriptors is this process's state, not the file's: an error
      // in both modes, never verdict 0 (which would queue the chunks for
      // re-download and overwrite).
      if (errno == EMFILE || errno == ENFILE)
        return fail(LBF_ERR_IO, std::string("cannot open ") + paths[f] + ": too many open files");
      // hash mode needs every file; verify mode leaves a missing file's chunks
      // '0' (Flood.cpp:257)
      if (!expected) return fail(LBF_ERR_IO, std::string("cannot open ") + paths[f]);
    }
    if (fd >= 0) posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    job.src.fds[f] = fd;
  }
  if (std::all_of(job.src.fds.begin(), job.src.fds.end(), [](int fd) { return fd < 0; })) {
    memset(out, 0, n);  // verify mode, no file there: every chunk stays '0'
    return LBF_OK;
  }
  job.file_of = file_of;
  job.offsets = offsets;
  job.sizes = sizes;
  job.expected = expected;
  if (expected) job.verdicts = out;
  else job.digests = out;
  return run_job(ctx, job, n);
}

}  // namespace

extern "C" int lbf_files_ranges(lbf_ctx* ctx, const char* const* paths, uint32_t n_files, const uint32_t* file_of,
                                const uint64_t* offsets, const uint32_t* sizes, uint64_t n, const uint8_t* expected,
                                uint8_t* out) {
  if (!ctx || !paths || n_files == 0) return fail(LBF_ERR_INVALID, "null context/paths or no file");
  if (n == 0) return LBF_OK;
  if (!offsets || !sizes || !out || (n_files > 1 && !file_of)) return fail(LBF_ERR_INVALID, "null argument");
  if (file_of)
    for (uint64_t i = 0; i < n; ++i)
      if (file_of[i] >= n_files) return fail(LBF_ERR_INVALID, "chunk " + std::to_string(i) + " names no file");
  for (uint32_t f = 0; f < n_files; ++f)
    if (!paths[f]) return fail(LBF_ERR_INVALID, "null path");
  const uint32_t window = files_window();
  if (n_files <= window || !file_of)
    return guarded([&] { return files_ranges_job(ctx, paths, n_files, file_of, offsets, sizes, n, expected, out); });
  // More files than may be open at once: one job per window of `window`
  // consecutive files, each over that window's chunks (gathered, then the
  // results scattered back to the caller's indices).
  return guarded([&]() -> int {
    const uint32_t n_win = (n_files + window - 1) / window;
    std::vector<std::vector<uint64_t>> members(n_win);
    for (uint64_t i = 0; i < n; ++i) members[file_of[i] / window].push_back(i);
    const size_t per = expected ? 1 : 20;
    std::vector<uint32_t> fo;
    std::vector<uint64_t> offs;
    std::vector<uint32_t> szs;
    std::vector<uint8_t> exp, res;
    for (uint32_t w = 0; w < n_win; ++w) {
      const std::vector<uint64_t>& idx = members[w];
      if (idx.empty()) continue;
      const uint32_t f0 = w * window, nf = std::min(window, n_files - f0);
      fo.resize(idx.size());
      offs.resize(idx.size());
      szs.resize(idx.size());
      res.assign(idx.size() * per, 0);
      if (expected) exp.resize(idx.size() * 20);
      for (size_t k = 0; k < idx.size(); ++k) {
        fo[k] = file_of[idx[k]] - f0;
        offs[k] = offsets[idx[k]];
        szs[k] = sizes[idx[k]];
        if (expected) memcpy(&exp[20 * k], expected + 20 * idx[k], 20);
      }
      if (int rc = files_ranges_job(ctx, paths + f0, nf, fo.data(), offs.data(), szs.data(), idx.size(),
                                    expected ? exp.data() : nullptr, res.data()))
        return rc;
      for (size_t k = 0; k < idx.size(); ++k) memcpy(out + per * idx[k], &res[per * k], per);
    }
    return LBF_OK;
  });
}

extern "C" int lbf_file_ranges(lbf_ctx* ctx, const char* path, const uint64_t* offsets, const uint32_t* sizes,
                               uint64_t n, const uint8_t* expected, uint8_t* out) {
  if (!ctx || !path) return fail(LBF_ERR_INVALID, "null context/path");
  return lbf_files_ranges(ctx, &path, 1, nullptr, offsets, sizes, n, expected, out);
}

extern "C" int lbf_sha1_one(lbf_ctx* ctx, const uint8_t* data, uint32_t size, uint8_t out[20]) {
  static const uint8_t kEmpty = 0;
  if (!data && size) return fail(LBF_ERR_INVALID, "null data");
  const uint64_t off = 0;
  return lbf_sha1_batch(ctx, data ? data : &kEmpty, size, &off, &size, 1, out, LBF_HOST_PTR);
}
