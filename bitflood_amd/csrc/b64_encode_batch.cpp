// b64_encode_batch.cpp -- lbf_b64_encode_update_batch: pieces of chunks in host
// memory encoded into the chunks' text slots and absorbed into caller-owned
// resumable state pairs (lbf_b64_enc_state, lbf_sha1_state), synchronously on
// worker 0's first stream.  What is refused, which characters a cut writes,
// where they lie on the device and how they come back is b64_encode_plan.hpp;
// the pieces are cut into launches and packed into copies by update_plan.hpp.
// Here the plan meets the stream: per launch one H2D per run of adjacent
// pieces, one of the touched state pairs and tables,
// lbf_b64_encode_update_launch, the tables back, then only the characters the
// launch produced.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "b64_encode_plan.hpp"
#include "lbf_host.hpp"

using namespace lbf;

namespace {

uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// The call's device memory: the update calls' one allocation on worker 0's
// device (current when this runs), grown on demand; the caller holds ctx->mu.
int encode_scratch(lbf_ctx* ctx, uint64_t need) {
  return grow_scratch(ctx->upd_dev, ctx->upd_cap, need, up(need, 1ull << 20), "lbf_b64_encode_update_batch");
}

struct EncodeCall {
  lbf_b64_enc_state* enc;
  lbf_sha1_state* sha;
  const uint32_t* state_of;
  const uint8_t* data;
  const uint64_t* offsets;
  const uint8_t* final_flags;
  const uint8_t* expected;
  uint8_t* verdicts;
  uint8_t* text;
  const uint64_t* text_offsets;
  const uint32_t* text_caps;
  uint64_t* new_offsets;
  uint32_t* new_lens;
  uint32_t* text_sizes;
};

// Below this many characters per run on average the text comes back as one
// copy of the launch's area and is scattered on the host (b64_update_batch.cpp's
// figure, as little measured here as there).
constexpr uint64_t kDirectRunBytes = 64 << 10;

// One launch: the cuts' state pairs, tables and bytes up, the kernels, states
// and results back into the caller's arrays.
int encode_run_launch(lbf_ctx* ctx, hipStream_t st, const EncodeCall& c, const std::vector<UpdateCut>& cuts) {
  const uint64_t m = cuts.size();
  if (m == 0) return LBF_OK;
  std::vector<Run> runs, back_runs;
  std::vector<uint64_t> data_off;
  const uint64_t data_area = update_runs(cuts, runs, data_off);
  std::vector<B64EncSpan> spans(m);
  std::vector<uint64_t> host_at(m), dev_at(m);
  std::vector<uint32_t> got(m);
  std::vector<uint8_t> fin(m);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece;
    const lbf_b64_enc_state& e = c.enc[update_state_of(c.state_of, i)];
    fin[k] = cuts[k].last && c.final_flags && c.final_flags[i] ? 1 : 0;
    spans[k] = b64_encode_span(e.taken, cuts[k].size, fin[k] != 0, e.layout == LBF_B64_LAYOUT_FLAT, c.text_caps[i]);
    host_at[k] = c.text_offsets[i] + spans[k].lo;
  }
  std::vector<B64EncPlace> places;
  const uint64_t text_area = b64_encode_places(spans, places);
  // one block of tables, up and back: encoder states | SHA states | piece offsets | slot starts | new offsets |
  // piece sizes | caps | new lengths | text lengths | expected | digests | final flags | verdicts
  const uint64_t sha_at = 16 * m, off_at = sha_at + 96 * m, slot_at = off_at + 8 * m, noff_at = slot_at + 8 * m,
                 size_at = noff_at + 8 * m, cap_at = size_at + 4 * m, nlen_at = cap_at + 4 * m,
                 tsize_at = nlen_at + 4 * m, exp_at = tsize_at + 4 * m, dig_at = exp_at + 20 * m,
                 fin_at = dig_at + 20 * m, ver_at = fin_at + m, tab_bytes = ver_at + m;
  std::vector<uint8_t> tab(tab_bytes, 0), chars;
  SyncOnExit sync{st};  // after the vectors the copies use: every exit waits for the stream before they go
  lbf_b64_enc_state* h_enc = reinterpret_cast<lbf_b64_enc_state*>(tab.data());
  lbf_sha1_state* h_sha = reinterpret_cast<lbf_sha1_state*>(tab.data() + sha_at);
  uint64_t* h_off = reinterpret_cast<uint64_t*>(tab.data() + off_at);
  uint64_t* h_slot = reinterpret_cast<uint64_t*>(tab.data() + slot_at);
  uint32_t* h_size = reinterpret_cast<uint32_t*>(tab.data() + size_at);
  uint32_t* h_cap = reinterpret_cast<uint32_t*>(tab.data() + cap_at);
  const uint32_t* h_nlen = reinterpret_cast<const uint32_t*>(tab.data() + nlen_at);
  const uint32_t* h_tsize = reinterpret_cast<const uint32_t*>(tab.data() + tsize_at);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece, s = update_state_of(c.state_of, i);
    h_enc[k] = c.enc[s];
    h_sha[k] = c.sha[s];
    h_off[k] = data_off[k];
    h_slot[k] = places[k].slot;
    h_size[k] = cuts[k].size;
    h_cap[k] = c.text_caps[i];
    if (c.expected) memcpy(tab.data() + exp_at + 20 * k, c.expected + 20 * i, 20);
    tab[fin_at + k] = fin[k];
  }
  // device layout: piece bytes | text | tables
  const uint64_t data_b = up(data_area + 16, 256), text_b = up(text_area + 16, 256);
  if (int rc = encode_scratch(ctx, data_b + text_b + up(tab_bytes, 256))) return rc;
  uint8_t* d_data = ctx->upd_dev;
  uint8_t* d_text = d_data + data_b;
  uint8_t* d_tab = d_text + text_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_data + r.dst, c.data + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  if (int rc = lbf_b64_encode_update_launch(
          reinterpret_cast<lbf_b64_enc_state*>(d_tab), reinterpret_cast<lbf_sha1_state*>(d_tab + sha_at), m, nullptr,
          d_data, reinterpret_cast<const uint64_t*>(d_tab + off_at), reinterpret_cast<const uint32_t*>(d_tab + size_at),
          d_tab + fin_at, m, reinterpret_cast<char*>(d_text), reinterpret_cast<const uint64_t*>(d_tab + slot_at),
          reinterpret_cast<const uint32_t*>(d_tab + cap_at), reinterpret_cast<uint64_t*>(d_tab + noff_at),
          reinterpret_cast<uint32_t*>(d_tab + nlen_at), reinterpret_cast<uint32_t*>(d_tab + tsize_at), d_tab + dig_at,
          c.expected ? d_tab + exp_at : nullptr, c.expected ? d_tab + ver_at : nullptr, st))
    return rc;
  LBF_HIP_TRY(hipMemcpyAsync(tab.data(), d_tab, tab.size(), hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  // the characters this launch produced, and only those
  uint64_t total = 0;
  for (uint64_t k = 0; k < m; ++k) {
    got[k] = h_nlen[k];
    dev_at[k] = places[k].dev;
    total += got[k];
    if (got[k] != places[k].room)
      return fail(LBF_ERR_HIP, "lbf_b64_encode_update_batch: a piece wrote other characters than planned (internal error)");
  }
  b64_encode_copyback(dev_at, host_at, got, back_runs);
  if (total && c.text) {
    if (total / back_runs.size() >= kDirectRunBytes) {
      for (const Run& r : back_runs)
        LBF_HIP_TRY(hipMemcpyAsync(c.text + r.dst, d_text + r.src, r.len, hipMemcpyDeviceToHost, st));
      LBF_HIP_TRY(hipStreamSynchronize(st));
    } else {
      chars.resize(text_area);
      LBF_HIP_TRY(hipMemcpyAsync(chars.data(), d_text, text_area, hipMemcpyDeviceToHost, st));
      LBF_HIP_TRY(hipStreamSynchronize(st));
      for (const Run& r : back_runs) memcpy(c.text + r.dst, chars.data() + r.src, r.len);
    }
  }
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece, s = update_state_of(c.state_of, i);
    c.enc[s] = h_enc[k];
    c.sha[s] = h_sha[k];
    const bool first = cuts[k].off == c.offsets[i];  // a cut piece reports where its first cut began and all it wrote
    if (c.new_offsets && first) c.new_offsets[i] = host_at[k];
    if (c.new_lens) c.new_lens[i] = (first ? 0u : c.new_lens[i]) + got[k];
    if (!fin[k]) continue;  // only final pieces report
    if (c.text_sizes) c.text_sizes[i] = h_tsize[k];
    if (c.verdicts) c.verdicts[i] = tab[ver_at + k];
  }
  return LBF_OK;
}

}  // namespace

extern "C" int lbf_b64_encode_update_batch(lbf_ctx* ctx, lbf_b64_enc_state* enc_states, lbf_sha1_state* sha_states,
                                           uint64_t n_states, const uint32_t* state_of, const uint8_t* data,
                                           uint64_t data_len, const uint64_t* offsets, const uint32_t* sizes,
                                           const uint8_t* final_flags, uint64_t n, const uint8_t* expected,
                                           uint8_t* verdicts, char* text, uint64_t text_len,
                                           const uint64_t* text_offsets, const uint32_t* text_caps,
                                           uint64_t* new_offsets, uint32_t* new_lens, uint32_t* text_sizes) {
  const std::string who = "lbf_b64_encode_update_batch";
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (!enc_states || !sha_states || !data || !offsets || !sizes || !text_offsets || !text_caps)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (!text && text_len) return fail(LBF_ERR_INVALID, who + ": text is null but text_len is not 0");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n too large");
  if ((verdicts != nullptr) != (expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  return guarded([&]() -> int {
    std::string why;
    const uint64_t bad = b64_encode_check(enc_states, sha_states, n_states, state_of, data_len, offsets, sizes, n,
                                          text ? text_len : 0, text_offsets, text_caps, why);
    if (bad != kNoPiece) return fail(LBF_ERR_INVALID, who + ": piece " + std::to_string(bad) + " " + why);
    const std::vector<std::vector<UpdateCut>> launches = update_launches(offsets, sizes, n, ctx->update_bytes);
    const EncodeCall call{enc_states, sha_states, state_of,     data,         offsets,   final_flags, expected,
                          verdicts,   reinterpret_cast<uint8_t*>(text), text_offsets, text_caps, new_offsets,
                          new_lens,   text_sizes};
    std::lock_guard<std::mutex> lock(ctx->mu);
    KeepCurrentDevice keep;
    Worker& w = ctx->workers[0];
    LBF_HIP_TRY(hipSetDevice(w.device));
    hipStream_t st = w.dev[0].stream;
    for (const std::vector<UpdateCut>& cuts : launches)
      if (int rc = encode_run_launch(ctx, st, call, cuts)) return rc;
    return (int)LBF_OK;
  });
}
