// update_batch.cpp -- lbf_sha1_update_batch: pieces of chunks in host memory
// absorbed into caller-owned resumable states (lbf_sha1_state), synchronously
// on worker 0's first stream.  What is refused, how a call is spread over
// launches and how a launch's bytes are packed is update_plan.hpp; here the
// plan meets the stream: per launch one H2D per run of adjacent pieces, one of
// the touched states and tables, the launch, one D2H of states and results.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "lbf_host.hpp"
#include "update_plan.hpp"

using namespace lbf;

namespace {

uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// The call's device memory: one allocation on worker 0's device (current when
// this runs), grown on demand; the caller holds ctx->mu.
int update_scratch(lbf_ctx* ctx, uint64_t need) {
  return grow_scratch(ctx->upd_dev, ctx->upd_cap, need, up(need, 1ull << 20), "lbf_sha1_update_batch");
}

struct UpdateCall {
  lbf_sha1_state* states;
  const uint32_t* state_of;
  const uint8_t* base;
  const uint8_t* final_flags;
  uint8_t* out_digests;
  const uint8_t* expected;
  uint8_t* verdicts;
};

// One launch: the cuts' states, tables and bytes up, the kernel, states and
// results back into the caller's arrays.
int update_run_launch(lbf_ctx* ctx, hipStream_t st, const UpdateCall& c, const std::vector<UpdateCut>& cuts) {
  const uint64_t m = cuts.size();
  if (m == 0) return LBF_OK;
  std::vector<Run> runs;
  std::vector<uint64_t> dev_off;
  const uint64_t area = update_runs(cuts, runs, dev_off);
  // inputs: states | offsets | sizes | expected | final flags; results: digests | verdicts
  const uint64_t st_b = 96 * m, off_at = st_b, size_at = off_at + 8 * m, exp_at = size_at + 4 * m,
                 fin_at = exp_at + 20 * m, in_bytes = fin_at + m;
  std::vector<uint8_t> in(in_bytes, 0), res(21 * m, 0);
  SyncOnExit sync{st};  // after the vectors the copies use: every exit waits for the stream before they go
  lbf_sha1_state* h_states = reinterpret_cast<lbf_sha1_state*>(in.data());
  uint64_t* h_off = reinterpret_cast<uint64_t*>(in.data() + off_at);
  uint32_t* h_size = reinterpret_cast<uint32_t*>(in.data() + size_at);
  bool any_final = false;
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece;
    h_states[k] = c.states[update_state_of(c.state_of, i)];
    h_off[k] = dev_off[k];
    h_size[k] = cuts[k].size;
    if (c.expected) memcpy(in.data() + exp_at + 20 * k, c.expected + 20 * i, 20);
    const bool fin = cuts[k].last && c.final_flags && c.final_flags[i];
    in[fin_at + k] = fin ? 1 : 0;
    any_final |= fin;
  }
  // device layout: bytes | inputs | results
  const uint64_t data_b = up(area + 16, 256), in_b = up(in_bytes, 256);
  if (int rc = update_scratch(ctx, data_b + in_b + up(21 * m, 256))) return rc;
  uint8_t* d_data = ctx->upd_dev;
  uint8_t* d_in = d_data + data_b;
  uint8_t* d_res = d_in + in_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_data + r.dst, c.base + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_in, in.data(), in.size(), hipMemcpyHostToDevice, st));
  uint8_t* d_dig = d_res;
  uint8_t* d_ver = d_res + 20 * m;
  if (int rc = lbf_sha1_update_launch(reinterpret_cast<lbf_sha1_state*>(d_in), m, nullptr, d_data,
                                      reinterpret_cast<const uint64_t*>(d_in + off_at),
                                      reinterpret_cast<const uint32_t*>(d_in + size_at), d_in + fin_at, m, d_dig,
                                      c.expected ? d_in + exp_at : nullptr, c.expected ? d_ver : nullptr, st))
    return rc;
  LBF_HIP_TRY(hipMemcpyAsync(in.data(), d_in, st_b, hipMemcpyDeviceToHost, st));
  if (any_final) LBF_HIP_TRY(hipMemcpyAsync(res.data(), d_res, res.size(), hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece;
    c.states[update_state_of(c.state_of, i)] = h_states[k];
    if (!in[fin_at + k]) continue;  // only final pieces report
    if (c.out_digests) memcpy(c.out_digests + 20 * i, res.data() + 20 * k, 20);
    if (c.verdicts) c.verdicts[i] = res[20 * m + k];
  }
  return LBF_OK;
}

}  // namespace

extern "C" int lbf_sha1_update_batch(lbf_ctx* ctx, lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                                     const uint8_t* base, uint64_t base_len, const uint64_t* offsets,
                                     const uint32_t* sizes, const uint8_t* final_flags, uint64_t n,
                                     uint8_t* out_digests, const uint8_t* expected, uint8_t* verdicts) {
  const char* who = "lbf_sha1_update_batch";
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (!states || !base || !offsets || !sizes) return fail(LBF_ERR_INVALID, std::string(who) + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, std::string(who) + ": n too large");
  if ((verdicts != nullptr) != (expected != nullptr))
    return fail(LBF_ERR_INVALID, std::string(who) + ": expected and verdicts go together");
  return guarded([&]() -> int {
    std::string why;
    const uint64_t bad = update_check(states, n_states, state_of, base_len, offsets, sizes, n, why);
    if (bad != kNoPiece) return fail(LBF_ERR_INVALID, std::string(who) + ": piece " + std::to_string(bad) + " " + why);
    const std::vector<std::vector<UpdateCut>> launches = update_launches(offsets, sizes, n, ctx->update_bytes);
    const UpdateCall call{states, state_of, base, final_flags, out_digests, expected, verdicts};
    std::lock_guard<std::mutex> lock(ctx->mu);
    KeepCurrentDevice keep;
    Worker& w = ctx->workers[0];
    LBF_HIP_TRY(hipSetDevice(w.device));
    hipStream_t st = w.dev[0].stream;
    for (const std::vector<UpdateCut>& cuts : launches)
      if (int rc = update_run_launch(ctx, st, call, cuts)) return rc;
    return (int)LBF_OK;
  });
}
