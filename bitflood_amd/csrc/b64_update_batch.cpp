// b64_update_batch.cpp -- lbf_b64_update_batch: pieces of chunks' base64 text
// in host memory decoded into the chunks' slots and absorbed into caller-owned
// resumable state pairs (lbf_b64_state, lbf_sha1_state), synchronously on
// worker 0's first stream.  What is refused, where a launch's decoded bytes lie
// on the device and how they come back is b64_update_plan.hpp; the text is cut
// into launches and packed into copies by update_plan.hpp.  Here the plan meets
// the stream: per launch one H2D per run of adjacent text pieces, one of the
// touched state pairs and tables, lbf_b64_update_launch (with two more tables:
// the characters of each piece the line path and the flat path took, for
// lbf_ctx_b64_update_stats and lbf_ctx_b64_flat_stats), the tables back, then
// only the bytes the launch decoded.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "b64_update_lines.hpp"
#include "b64_update_plan.hpp"
#include "lbf_host.hpp"

using namespace lbf;

namespace {

uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// The call's device memory: the update calls' one allocation on worker 0's
// device (current when this runs), grown on demand; the caller holds ctx->mu.
int text_scratch(lbf_ctx* ctx, uint64_t need) {
  return grow_scratch(ctx->upd_dev, ctx->upd_cap, need, up(need, 1ull << 20), "lbf_b64_update_batch");
}

struct TextCall {
  lbf_b64_state* b64;
  lbf_sha1_state* sha;
  const uint32_t* state_of;
  const uint8_t* text;
  const uint8_t* final_flags;
  const uint32_t* caps;
  const uint8_t* expected;
  uint8_t* out;
  const uint64_t* out_offsets;
  uint32_t* out_sizes;
  uint8_t* verdicts;
};

// Below this many bytes per run on average the decoded bytes come back as one
// copy of the launch's area and are scattered on the host, so that thousands of
// small pieces do not cost a copy each.  The figure is a guess, not a measured
// crossover.
constexpr uint64_t kDirectRunBytes = 64 << 10;

// One launch: the cuts' state pairs, tables and text up, the kernels,
// states and results back into the caller's arrays.
int text_run_launch(lbf_ctx* ctx, hipStream_t st, const TextCall& c, const std::vector<UpdateCut>& cuts) {
  const uint64_t m = cuts.size();
  if (m == 0) return LBF_OK;
  std::vector<Run> runs, back_runs;
  std::vector<uint64_t> text_off;
  const uint64_t text_area = update_runs(cuts, runs, text_off);
  std::vector<uint64_t> decoded(m), host_at(m), dev_at(m);
  std::vector<uint32_t> ncarry(m), len(m), cap(m), got(m);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece;
    const lbf_b64_state& b = c.b64[update_state_of(c.state_of, i)];
    decoded[k] = b.decoded;
    ncarry[k] = b.ncarry;
    len[k] = cuts[k].size;
    cap[k] = c.caps[i];
    host_at[k] = c.out_offsets[i] + std::min<uint64_t>(b.decoded, cap[k]);
  }
  std::vector<B64Place> places;
  const uint64_t out_area = b64_update_places(decoded, ncarry, len, cap, places);
  // one block of tables, up and back: b64 states | SHA states | text offsets |
  // slot starts | piece offsets | text lengths | chunk sizes | piece sizes |
  // decoded lengths | line-path characters | flat-path characters | expected | digests | final flags | verdicts
  const uint64_t sha_at = 16 * m, toff_at = sha_at + 96 * m, slot_at = toff_at + 8 * m, poff_at = slot_at + 8 * m,
                 tlen_at = poff_at + 8 * m, cap_at = tlen_at + 4 * m, psize_at = cap_at + 4 * m,
                 osize_at = psize_at + 4 * m, lines_at = osize_at + 4 * m, flat_at = lines_at + 4 * m,
                 exp_at = flat_at + 4 * m,
                 dig_at = exp_at + 20 * m, fin_at = dig_at + 20 * m, ver_at = fin_at + m, tab_bytes = ver_at + m;
  std::vector<uint8_t> tab(tab_bytes, 0), bytes;
  SyncOnExit sync{st};  // after the vectors the copies use: every exit waits for the stream before they go
  lbf_b64_state* h_b64 = reinterpret_cast<lbf_b64_state*>(tab.data());
  lbf_sha1_state* h_sha = reinterpret_cast<lbf_sha1_state*>(tab.data() + sha_at);
  uint64_t* h_toff = reinterpret_cast<uint64_t*>(tab.data() + toff_at);
  uint64_t* h_slot = reinterpret_cast<uint64_t*>(tab.data() + slot_at);
  uint32_t* h_tlen = reinterpret_cast<uint32_t*>(tab.data() + tlen_at);
  uint32_t* h_cap = reinterpret_cast<uint32_t*>(tab.data() + cap_at);
  const uint32_t* h_psize = reinterpret_cast<const uint32_t*>(tab.data() + psize_at);
  const uint32_t* h_osize = reinterpret_cast<const uint32_t*>(tab.data() + osize_at);
  const uint32_t* h_lines = reinterpret_cast<const uint32_t*>(tab.data() + lines_at);  // zero on the way up
  const uint32_t* h_flat = reinterpret_cast<const uint32_t*>(tab.data() + flat_at);    // as well
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece, s = update_state_of(c.state_of, i);
    h_b64[k] = c.b64[s];
    h_sha[k] = c.sha[s];
    h_toff[k] = text_off[k];
    h_slot[k] = places[k].slot;
    h_tlen[k] = len[k];
    h_cap[k] = cap[k];
    if (c.expected) memcpy(tab.data() + exp_at + 20 * k, c.expected + 20 * i, 20);
    tab[fin_at + k] = cuts[k].last && c.final_flags && c.final_flags[i] ? 1 : 0;
  }
  // device layout: text | decoded bytes | tables
  const uint64_t text_b = up(text_area + 16, 256), out_b = up(out_area + 16, 256);
  if (int rc = text_scratch(ctx, text_b + out_b + up(tab_bytes, 256))) return rc;
  uint8_t* d_text = ctx->upd_dev;
  uint8_t* d_out = d_text + text_b;
  uint8_t* d_tab = d_out + out_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_text + r.dst, c.text + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  if (int rc = b64_update_launch_counted(
          reinterpret_cast<lbf_b64_state*>(d_tab), reinterpret_cast<lbf_sha1_state*>(d_tab + sha_at), m, nullptr,
          reinterpret_cast<const char*>(d_text), reinterpret_cast<const uint64_t*>(d_tab + toff_at),
          reinterpret_cast<const uint32_t*>(d_tab + tlen_at), d_tab + fin_at, m, d_out,
          reinterpret_cast<const uint64_t*>(d_tab + slot_at), reinterpret_cast<const uint32_t*>(d_tab + cap_at),
          reinterpret_cast<uint32_t*>(d_tab + osize_at), d_tab + dig_at, c.expected ? d_tab + exp_at : nullptr,
          c.expected ? d_tab + ver_at : nullptr, reinterpret_cast<uint64_t*>(d_tab + poff_at),
          reinterpret_cast<uint32_t*>(d_tab + psize_at), reinterpret_cast<uint32_t*>(d_tab + lines_at),
          reinterpret_cast<uint32_t*>(d_tab + flat_at), st))
    return rc;
  LBF_HIP_TRY(hipMemcpyAsync(tab.data(), d_tab, tab.size(), hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  // the bytes this launch decoded, and only those
  uint64_t total = 0;
  for (uint64_t k = 0; k < m; ++k) {
    const uint32_t by_lines = std::min(h_lines[k], len[k]);
    ctx->b64_line_chars += by_lines;
    ctx->b64_scan_chars += len[k] - by_lines;
    ctx->b64_flat_chars += std::min(h_flat[k], len[k] - by_lines);  // a share of the scan path's count
    got[k] = h_psize[k];
    dev_at[k] = places[k].dev;
    total += got[k];
    if (got[k] > places[k].room)
      return fail(LBF_ERR_HIP, "lbf_b64_update_batch: a piece decoded past its bound (internal error)");
  }
  b64_update_copyback(dev_at, host_at, got, back_runs);
  if (total && c.out) {
    if (total / back_runs.size() >= kDirectRunBytes) {
      for (const Run& r : back_runs)
        LBF_HIP_TRY(hipMemcpyAsync(c.out + r.dst, d_out + r.src, r.len, hipMemcpyDeviceToHost, st));
      LBF_HIP_TRY(hipStreamSynchronize(st));
    } else {
      bytes.resize(out_area);
      LBF_HIP_TRY(hipMemcpyAsync(bytes.data(), d_out, out_area, hipMemcpyDeviceToHost, st));
      LBF_HIP_TRY(hipStreamSynchronize(st));
      for (const Run& r : back_runs) memcpy(c.out + r.dst, bytes.data() + r.src, r.len);
    }
  }
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece, s = update_state_of(c.state_of, i);
    c.b64[s] = h_b64[k];
    c.sha[s] = h_sha[k];
    if (!tab[fin_at + k]) continue;  // only final pieces report
    if (c.out_sizes) c.out_sizes[i] = h_osize[k];
    if (c.verdicts) c.verdicts[i] = tab[ver_at + k];
  }
  return LBF_OK;
}

}  // namespace

extern "C" int lbf_b64_update_batch(lbf_ctx* ctx, lbf_b64_state* b64_states, lbf_sha1_state* sha_states,
                                    uint64_t n_states, const uint32_t* state_of, const char* text, uint64_t text_len,
                                    const uint64_t* text_offsets, const uint32_t* text_lens,
                                    const uint8_t* final_flags, uint64_t n, const uint32_t* expected_sizes,
                                    const uint8_t* expected, uint8_t* out, uint64_t out_len,
                                    const uint64_t* out_offsets, uint32_t* out_sizes, uint8_t* verdicts) {
  const std::string who = "lbf_b64_update_batch";
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (!b64_states || !sha_states || !text || !text_offsets || !text_lens || !expected_sizes || !out_offsets)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (!out && out_len) return fail(LBF_ERR_INVALID, who + ": out is null but out_len is not 0");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n too large");
  if ((verdicts != nullptr) != (expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  return guarded([&]() -> int {
    std::string why;
    const uint64_t bad = b64_update_check(b64_states, sha_states, n_states, state_of, text_len, text_offsets,
                                          text_lens, n, expected_sizes, out_len, out_offsets, why);
    if (bad != kNoPiece) return fail(LBF_ERR_INVALID, who + ": piece " + std::to_string(bad) + " " + why);
    const std::vector<std::vector<UpdateCut>> launches = update_launches(text_offsets, text_lens, n, ctx->update_bytes);
    const TextCall call{b64_states, sha_states,  state_of, reinterpret_cast<const uint8_t*>(text), final_flags,
                        expected_sizes, expected, out, out_offsets, out_sizes, verdicts};
    std::lock_guard<std::mutex> lock(ctx->mu);
    KeepCurrentDevice keep;
    Worker& w = ctx->workers[0];
    LBF_HIP_TRY(hipSetDevice(w.device));
    hipStream_t st = w.dev[0].stream;
    for (const std::vector<UpdateCut>& cuts : launches)
      if (int rc = text_run_launch(ctx, st, call, cuts)) return rc;
    return (int)LBF_OK;
  });
}
