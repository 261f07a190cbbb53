// update_host.hpp -- what the piecewise host calls share where the plan meets
// the stream (update_batch.cpp: hash and text; b64_encode_batch.cpp: encode):
// how a call begins, the calls' one device allocation, and how what a launch
// produced comes back.
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "lbf_host.hpp"
#include "update_plan.hpp"

namespace lbf {

// One call from its first refusal to its last launch, synchronously on worker
// 0's first stream.  `null_argument` and `other` (a refusal of the call's own
// that stands between "null argument" and "n too large", or null) are the
// caller's tests of its arguments; check(why) is the planner's verdict on the
// call and launch(stream, cuts) one launch of it.
template <class Check, class Launch>
int update_call(lbf_ctx* ctx, const std::string& who, uint64_t n, bool null_argument, const char* other,
                const void* expected, const void* verdicts, const uint64_t* offsets, const uint32_t* sizes,
                Check&& check, Launch&& launch) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (null_argument) return fail(LBF_ERR_INVALID, who + ": null argument");
  if (other) return fail(LBF_ERR_INVALID, who + ": " + other);
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n too large");
  if ((verdicts != nullptr) != (expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  return guarded([&]() -> int {
    std::string why;
    const uint64_t bad = check(why);
    if (bad != kNoPiece) return fail(LBF_ERR_INVALID, who + ": piece " + std::to_string(bad) + " " + why);
    const std::vector<std::vector<UpdateCut>> launches = update_launches(offsets, sizes, n, ctx->update_bytes);
    std::lock_guard<std::mutex> lock(ctx->mu);
    KeepCurrentDevice keep;
    Worker& w = ctx->workers[0];
    LBF_HIP_TRY(hipSetDevice(w.device));
    hipStream_t st = w.dev[0].stream;
    for (const std::vector<UpdateCut>& cuts : launches)
      if (int rc = launch(st, cuts)) return rc;
    return (int)LBF_OK;
  });
}

// The calls' device memory: one allocation on worker 0's device (current when
// this runs), grown on demand; the caller holds ctx->mu.
inline int update_scratch(lbf_ctx* ctx, uint64_t need, const char* who) {
  return grow_scratch(ctx->upd_dev, ctx->upd_cap, need, round_up(need, 1ull << 20), who);
}

// The `total` bytes a launch produced in its device area of `area` bytes at
// d_src, to where `runs` (copyback_runs) say they belong in host_dst: a copy
// per run, or below kDirectRunBytes per run one copy of the area and a scatter
// on the host.  Returns with the bytes in place.
inline int copy_back(hipStream_t st, const std::vector<Run>& runs, uint64_t total, uint64_t area, const uint8_t* d_src,
                     uint8_t* host_dst) {
  if (!total || !host_dst) return LBF_OK;
  if (total / runs.size() >= kDirectRunBytes) {
    for (const Run& r : runs)
      LBF_HIP_TRY(hipMemcpyAsync(host_dst + r.dst, d_src + r.src, r.len, hipMemcpyDeviceToHost, st));
    LBF_HIP_TRY(hipStreamSynchronize(st));
    return LBF_OK;
  }
  std::vector<uint8_t> bytes(area);
  LBF_HIP_TRY(hipMemcpyAsync(bytes.data(), d_src, area, hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  for (const Run& r : runs) memcpy(host_dst + r.dst, bytes.data() + r.src, r.len);
  return LBF_OK;
}

}  // namespace lbf
