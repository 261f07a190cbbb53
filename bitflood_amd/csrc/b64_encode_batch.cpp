// b64_encode_batch.cpp -- lbf_b64_encode_update_batch: pieces of chunks in host
// memory encoded into the chunks' text slots and absorbed into caller-owned
// resumable state pairs (lbf_b64_enc_state, lbf_sha1_state), synchronously on
// worker 0's first stream.  What is refused, which characters a cut writes,
// where they and the launch's tables lie on the device is b64_encode_plan.hpp;
// the pieces are cut into launches and packed into copies by update_plan.hpp;
// how a call begins and how characters come back is update_host.hpp.
// Here the plan meets the stream: per launch one H2D per run of adjacent
// pieces, one of the touched state pairs and tables,
// lbf_b64_encode_update_launch, the tables back, then only the characters the
// launch produced.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "b64_encode_plan.hpp"
#include "update_host.hpp"

using namespace lbf;

namespace {

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
  const EncodeTables at = encode_tables(m);  // one block of tables, up and back
  std::vector<uint8_t> tab(at.bytes, 0);
  SyncOnExit sync{st};  // after the vectors the copies use: every exit waits for the stream before they go
  lbf_b64_enc_state* h_enc = reinterpret_cast<lbf_b64_enc_state*>(tab.data() + at.enc);
  lbf_sha1_state* h_sha = reinterpret_cast<lbf_sha1_state*>(tab.data() + at.sha);
  uint64_t* h_off = reinterpret_cast<uint64_t*>(tab.data() + at.off);
  uint64_t* h_slot = reinterpret_cast<uint64_t*>(tab.data() + at.slot);
  uint32_t* h_size = reinterpret_cast<uint32_t*>(tab.data() + at.size);
  uint32_t* h_cap = reinterpret_cast<uint32_t*>(tab.data() + at.cap);
  const uint32_t* h_nlen = reinterpret_cast<const uint32_t*>(tab.data() + at.nlen);
  const uint32_t* h_tsize = reinterpret_cast<const uint32_t*>(tab.data() + at.tsize);
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece, s = update_state_of(c.state_of, i);
    h_enc[k] = c.enc[s];
    h_sha[k] = c.sha[s];
    h_off[k] = data_off[k];
    h_slot[k] = places[k].slot;
    h_size[k] = cuts[k].size;
    h_cap[k] = c.text_caps[i];
    if (c.expected) memcpy(tab.data() + at.exp + 20 * k, c.expected + 20 * i, 20);
    tab[at.fin + k] = fin[k];
  }
  // device layout: piece bytes | text | tables
  const uint64_t data_b = round_up(data_area + 16, 256), text_b = round_up(text_area + 16, 256);
  if (int rc = update_scratch(ctx, data_b + text_b + round_up(at.bytes, 256), "lbf_b64_encode_update_batch"))
    return rc;
  uint8_t* d_data = ctx->upd_dev;
  uint8_t* d_text = d_data + data_b;
  uint8_t* d_tab = d_text + text_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_data + r.dst, c.data + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  if (int rc = lbf_b64_encode_update_launch(
          reinterpret_cast<lbf_b64_enc_state*>(d_tab + at.enc), reinterpret_cast<lbf_sha1_state*>(d_tab + at.sha), m,
          nullptr, d_data, reinterpret_cast<const uint64_t*>(d_tab + at.off),
          reinterpret_cast<const uint32_t*>(d_tab + at.size), d_tab + at.fin, m, reinterpret_cast<char*>(d_text),
          reinterpret_cast<const uint64_t*>(d_tab + at.slot), reinterpret_cast<const uint32_t*>(d_tab + at.cap),
          reinterpret_cast<uint64_t*>(d_tab + at.noff), reinterpret_cast<uint32_t*>(d_tab + at.nlen),
          reinterpret_cast<uint32_t*>(d_tab + at.tsize), d_tab + at.dig, c.expected ? d_tab + at.exp : nullptr,
          c.expected ? d_tab + at.ver : nullptr, st))
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
  copyback_runs(dev_at, host_at, got, back_runs);
  if (int rc = copy_back(st, back_runs, total, text_area, d_text, c.text)) return rc;
  for (uint64_t k = 0; k < m; ++k) {
    const uint64_t i = cuts[k].piece, s = update_state_of(c.state_of, i);
    c.enc[s] = h_enc[k];
    c.sha[s] = h_sha[k];
    const bool first = cuts[k].off == c.offsets[i];  // a cut piece reports where its first cut began and all it wrote
    if (c.new_offsets && first) c.new_offsets[i] = host_at[k];
    if (c.new_lens) c.new_lens[i] = (first ? 0u : c.new_lens[i]) + got[k];
    if (!fin[k]) continue;  // only final pieces report
    if (c.text_sizes) c.text_sizes[i] = h_tsize[k];
    if (c.verdicts) c.verdicts[i] = tab[at.ver + k];
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
  const EncodeCall call{enc_states, sha_states, state_of,     data,         offsets,   final_flags, expected,
                        verdicts,   reinterpret_cast<uint8_t*>(text), text_offsets, text_caps, new_offsets,
                        new_lens,   text_sizes};
  return update_call(
      ctx, "lbf_b64_encode_update_batch", n,
      !enc_states || !sha_states || !data || !offsets || !sizes || !text_offsets || !text_caps,
      !text && text_len ? "text is null but text_len is not 0" : nullptr, expected, verdicts, offsets, sizes,
      [&](std::string& why) {
        return b64_encode_check(enc_states, sha_states, n_states, state_of, data_len, offsets, sizes, n,
                                text ? text_len : 0, text_offsets, text_caps, why);
      },
      [&](hipStream_t st, const std::vector<UpdateCut>& cuts) { return encode_run_launch(ctx, st, call, cuts); });
}
