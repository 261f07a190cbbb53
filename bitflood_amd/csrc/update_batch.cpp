// update_batch.cpp -- the piecewise host calls for hash and text:
// lbf_sha1_update_batch and lbf_b64_update_batch (one piece per state and
// call), lbf_sha1_update_seq_batch and lbf_b64_update_seq_batch (several pieces
// of one state, absorbed in the caller's order), all synchronously on worker
// 0's first stream.  What is refused, how a call is spread over launches, how a
// launch's bytes are packed, how its cuts are grouped into chains and where its
// tables and decoded bytes lie is update_plan.hpp and b64_update_plan.hpp; how a
// call begins and how bytes come back is update_host.hpp.  Here the plan meets
// the stream: per launch one H2D per run of adjacent pieces, one of the touched
// states and tables, the device launch, the states and results back, for text
// then only the bytes the launch decoded.
//
// A launch always works through a chain table.  A touched state (pair) travels
// once, whatever the number of its pieces, and the pieces' tables go up in
// table order and come back to the caller's piece indices.  For the one-piece
// calls the table is the identity (no state repeats: checked), no chain_first
// goes up, and the device launch is the one that maps a lane or workgroup to a
// piece; the seq calls upload the table and enqueue the launch that walks a
// chain (slower at one piece per chain, DESIGN.md §4.9, so neither call is
// routed through the other's kernels).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "b64_update_lines.hpp"
#include "b64_update_plan.hpp"
#include "update_host.hpp"

using namespace lbf;

namespace {

struct UpdateCall {
  const char* who;
  bool seq;
  lbf_sha1_state* states;
  const uint32_t* state_of;
  const uint8_t* base;
  const uint8_t* final_flags;
  uint8_t* out_digests;
  const uint8_t* expected;
  uint8_t* verdicts;
};

// One launch of a hash call: the chains' states, the tables and the bytes up,
// the kernel, states and results back into the caller's arrays.
int hash_run_launch(lbf_ctx* ctx, hipStream_t st, const UpdateCall& c, const std::vector<UpdateCut>& cuts) {
  const uint64_t m = cuts.size();
  if (m == 0) return LBF_OK;
  std::vector<Run> runs;
  std::vector<uint64_t> dev_off;
  const uint64_t area = update_runs(cuts, runs, dev_off);
  const ChainTable t = table_of(cuts, c.state_of, c.seq);
  const uint64_t nc = t.chains();
  const HashTables at = hash_tables(m, nc, c.seq);
  std::vector<uint8_t> in(at.bytes, 0), res(21 * m, 0);  // results: digests | verdicts
  SyncOnExit sync{st};  // after the vectors the copies use: every exit waits for the stream before they go
  lbf_sha1_state* h_states = reinterpret_cast<lbf_sha1_state*>(in.data() + at.states);
  uint64_t* h_off = reinterpret_cast<uint64_t*>(in.data() + at.off);
  uint32_t* h_size = reinterpret_cast<uint32_t*>(in.data() + at.size);
  for (uint64_t ch = 0; ch < nc; ++ch) h_states[ch] = c.states[t.chain_id[ch]];
  if (c.seq) memcpy(in.data() + at.first, t.first.data(), 4 * (nc + 1));
  bool any_final = false;
  for (uint64_t j = 0; j < m; ++j) {  // table position j holds cut order[j]
    const UpdateCut& cut = cuts[t.order[j]];
    h_off[j] = dev_off[t.order[j]];
    h_size[j] = cut.size;
    if (c.expected) memcpy(in.data() + at.exp + 20 * j, c.expected + 20 * cut.piece, 20);
    const bool fin = cut.last && c.final_flags && c.final_flags[cut.piece];
    in[at.fin + j] = fin ? 1 : 0;
    any_final |= fin;
  }
  // device layout: bytes | inputs | results
  const uint64_t data_b = round_up(area + 16, 256), in_b = round_up(at.bytes, 256);
  if (int rc = update_scratch(ctx, data_b + in_b + round_up(21 * m, 256), c.who)) return rc;
  uint8_t* d_data = ctx->upd_dev;
  uint8_t* d_in = d_data + data_b;
  uint8_t* d_res = d_in + in_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_data + r.dst, c.base + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_in, in.data(), in.size(), hipMemcpyHostToDevice, st));
  lbf_sha1_state* d_states = reinterpret_cast<lbf_sha1_state*>(d_in + at.states);
  const uint64_t* d_off = reinterpret_cast<const uint64_t*>(d_in + at.off);
  const uint32_t* d_size = reinterpret_cast<const uint32_t*>(d_in + at.size);
  uint8_t* d_dig = d_res;
  const uint8_t* d_exp = c.expected ? d_in + at.exp : nullptr;
  uint8_t* d_ver = c.expected ? d_res + 20 * m : nullptr;
  if (int rc = c.seq ? lbf_sha1_update_seq_launch(d_states, nc, nullptr,
                                                  reinterpret_cast<const uint32_t*>(d_in + at.first), nc, d_data, d_off,
                                                  d_size, d_in + at.fin, m, d_dig, d_exp, d_ver, st)
                     : lbf_sha1_update_launch(d_states, m, nullptr, d_data, d_off, d_size, d_in + at.fin, m, d_dig,
                                              d_exp, d_ver, st))
    return rc;
  LBF_HIP_TRY(hipMemcpyAsync(in.data(), d_in, 96 * nc, hipMemcpyDeviceToHost, st));
  if (any_final) LBF_HIP_TRY(hipMemcpyAsync(res.data(), d_res, res.size(), hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  for (uint64_t ch = 0; ch < nc; ++ch) c.states[t.chain_id[ch]] = h_states[ch];
  for (uint64_t j = 0; j < m; ++j) {
    if (!in[at.fin + j]) continue;  // only final pieces report
    const uint64_t i = cuts[t.order[j]].piece;
    if (c.out_digests) memcpy(c.out_digests + 20 * i, res.data() + 20 * j, 20);
    if (c.verdicts) c.verdicts[i] = res[20 * m + j];
  }
  return LBF_OK;
}

int hash_call(const char* who, bool seq, lbf_ctx* ctx, lbf_sha1_state* states, uint64_t n_states,
              const uint32_t* state_of, const uint8_t* base, uint64_t base_len, const uint64_t* offsets,
              const uint32_t* sizes, const uint8_t* final_flags, uint64_t n, uint8_t* out_digests,
              const uint8_t* expected, uint8_t* verdicts) {
  const UpdateCall call{who, seq, states, state_of, base, final_flags, out_digests, expected, verdicts};
  return update_call(
      ctx, who, n, !states || !base || !offsets || !sizes, nullptr, expected, verdicts, offsets, sizes,
      [&](std::string& why) {
        return seq ? update_seq_check(states, n_states, state_of, base_len, offsets, sizes, final_flags, n, why)
                   : update_check(states, n_states, state_of, base_len, offsets, sizes, n, why);
      },
      [&](hipStream_t st, const std::vector<UpdateCut>& cuts) { return hash_run_launch(ctx, st, call, cuts); });
}

struct TextCall {
  const char* who;
  bool seq;
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

// One launch of a text call: the chains' state pairs, the tables and the text
// up, the kernels (with two more tables: the characters of each piece the line
// path and the flat path took, for lbf_ctx_b64_update_stats and
// lbf_ctx_b64_flat_stats), states and results back into the caller's arrays,
// then one range of decoded bytes per chain.
int text_run_launch(lbf_ctx* ctx, hipStream_t st, const TextCall& c, const std::vector<UpdateCut>& cuts) {
  const uint64_t m = cuts.size();
  if (m == 0) return LBF_OK;
  std::vector<Run> runs, back_runs;
  std::vector<uint64_t> text_off;
  const uint64_t text_area = update_runs(cuts, runs, text_off);
  const ChainTable t = table_of(cuts, c.state_of, c.seq);
  const uint64_t nc = t.chains();
  // per chain: where it stands, its slot (the same for all its pieces: checked), the launch's characters of it
  std::vector<uint64_t> decoded(nc), chars(nc, 0), host_at(nc), dev_at(nc);
  std::vector<uint32_t> ncarry(nc), cap(nc), got(nc, 0);
  for (uint64_t ch = 0; ch < nc; ++ch) {
    const uint64_t i = cuts[t.order[t.first[ch]]].piece;
    const lbf_b64_state& b = c.b64[t.chain_id[ch]];
    decoded[ch] = b.decoded;
    ncarry[ch] = b.ncarry;
    cap[ch] = c.caps[i];
    host_at[ch] = c.out_offsets[i] + std::min<uint64_t>(b.decoded, cap[ch]);
    for (uint32_t j = t.first[ch]; j < t.first[ch + 1]; ++j) chars[ch] += cuts[t.order[j]].size;
  }
  std::vector<B64Place> places;
  const uint64_t out_area = b64_update_places(decoded, ncarry, chars, cap, places);
  const TextTables at = text_tables(m, nc, c.seq);  // one block of tables, up and back
  std::vector<uint8_t> tab(at.bytes, 0);
  SyncOnExit sync{st};  // after the vectors the copies use: every exit waits for the stream before they go
  lbf_b64_state* h_b64 = reinterpret_cast<lbf_b64_state*>(tab.data() + at.b64);
  lbf_sha1_state* h_sha = reinterpret_cast<lbf_sha1_state*>(tab.data() + at.sha);
  uint64_t* h_toff = reinterpret_cast<uint64_t*>(tab.data() + at.toff);
  uint64_t* h_slot = reinterpret_cast<uint64_t*>(tab.data() + at.slot);
  uint32_t* h_tlen = reinterpret_cast<uint32_t*>(tab.data() + at.tlen);
  uint32_t* h_cap = reinterpret_cast<uint32_t*>(tab.data() + at.cap);
  const uint32_t* h_psize = reinterpret_cast<const uint32_t*>(tab.data() + at.psize);
  const uint32_t* h_osize = reinterpret_cast<const uint32_t*>(tab.data() + at.osize);
  const uint32_t* h_lines = reinterpret_cast<const uint32_t*>(tab.data() + at.lines);  // zero on the way up
  const uint32_t* h_flat = reinterpret_cast<const uint32_t*>(tab.data() + at.flat);    // as well
  if (c.seq) memcpy(tab.data() + at.first, t.first.data(), 4 * (nc + 1));
  for (uint64_t ch = 0; ch < nc; ++ch) {
    h_b64[ch] = c.b64[t.chain_id[ch]];
    h_sha[ch] = c.sha[t.chain_id[ch]];
    for (uint32_t j = t.first[ch]; j < t.first[ch + 1]; ++j) {  // table position j holds cut order[j]
      const UpdateCut& cut = cuts[t.order[j]];
      h_toff[j] = text_off[t.order[j]];
      h_slot[j] = places[ch].slot;
      h_tlen[j] = cut.size;
      h_cap[j] = cap[ch];
      if (c.expected) memcpy(tab.data() + at.exp + 20 * j, c.expected + 20 * cut.piece, 20);
      tab[at.fin + j] = cut.last && c.final_flags && c.final_flags[cut.piece] ? 1 : 0;
    }
  }
  // device layout: text | decoded bytes | tables
  const uint64_t text_b = round_up(text_area + 16, 256), out_b = round_up(out_area + 16, 256);
  if (int rc = update_scratch(ctx, text_b + out_b + round_up(at.bytes, 256), c.who)) return rc;
  uint8_t* d_text = ctx->upd_dev;
  uint8_t* d_out = d_text + text_b;
  uint8_t* d_tab = d_out + out_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_text + r.dst, c.text + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  lbf_b64_state* d_b64 = reinterpret_cast<lbf_b64_state*>(d_tab + at.b64);
  lbf_sha1_state* d_sha = reinterpret_cast<lbf_sha1_state*>(d_tab + at.sha);
  const char* d_chars = reinterpret_cast<const char*>(d_text);
  const uint64_t* d_toff = reinterpret_cast<const uint64_t*>(d_tab + at.toff);
  const uint32_t* d_tlen = reinterpret_cast<const uint32_t*>(d_tab + at.tlen);
  const uint64_t* d_slot = reinterpret_cast<const uint64_t*>(d_tab + at.slot);
  const uint32_t* d_cap = reinterpret_cast<const uint32_t*>(d_tab + at.cap);
  uint32_t* d_osize = reinterpret_cast<uint32_t*>(d_tab + at.osize);
  const uint8_t* d_exp = c.expected ? d_tab + at.exp : nullptr;
  uint8_t* d_ver = c.expected ? d_tab + at.ver : nullptr;
  uint64_t* d_poff = reinterpret_cast<uint64_t*>(d_tab + at.poff);
  uint32_t* d_psize = reinterpret_cast<uint32_t*>(d_tab + at.psize);
  uint32_t* d_lines = reinterpret_cast<uint32_t*>(d_tab + at.lines);
  uint32_t* d_flat = reinterpret_cast<uint32_t*>(d_tab + at.flat);
  if (int rc = c.seq ? b64_update_seq_launch_counted(d_b64, d_sha, nc, nullptr,
                                                     reinterpret_cast<const uint32_t*>(d_tab + at.first), nc, d_chars,
                                                     d_toff, d_tlen, d_tab + at.fin, m, d_out, d_slot, d_cap, d_osize,
                                                     d_tab + at.dig, d_exp, d_ver, d_poff, d_psize, d_lines, d_flat, st)
                     : b64_update_launch_counted(d_b64, d_sha, m, nullptr, d_chars, d_toff, d_tlen, d_tab + at.fin, m,
                                                 d_out, d_slot, d_cap, d_osize, d_tab + at.dig, d_exp, d_ver, d_poff,
                                                 d_psize, d_lines, d_flat, st))
    return rc;
  LBF_HIP_TRY(hipMemcpyAsync(tab.data(), d_tab, tab.size(), hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  // the bytes this launch decoded, and only those: a chain's pieces decode to one range
  uint64_t total = 0;
  for (uint64_t ch = 0; ch < nc; ++ch) {
    uint64_t sum = 0;
    for (uint32_t j = t.first[ch]; j < t.first[ch + 1]; ++j) {
      const uint32_t len = h_tlen[j];
      const uint32_t by_lines = std::min(h_lines[j], len);
      ctx->b64_line_chars += by_lines;
      ctx->b64_scan_chars += len - by_lines;
      ctx->b64_flat_chars += std::min(h_flat[j], len - by_lines);  // a share of the scan path's count
      sum += h_psize[j];
    }
    if (sum > places[ch].room)
      return fail(LBF_ERR_HIP, std::string(c.who) + (c.seq ? ": a chain" : ": a piece") +
                                   " decoded past its bound (internal error)");
    got[ch] = (uint32_t)sum;  // at most the chunk's size
    dev_at[ch] = places[ch].dev;
    total += sum;
  }
  copyback_runs(dev_at, host_at, got, back_runs);
  if (int rc = copy_back(st, back_runs, total, out_area, d_out, c.out)) return rc;
  for (uint64_t ch = 0; ch < nc; ++ch) {
    c.b64[t.chain_id[ch]] = h_b64[ch];
    c.sha[t.chain_id[ch]] = h_sha[ch];
  }
  for (uint64_t j = 0; j < m; ++j) {
    if (!tab[at.fin + j]) continue;  // only final pieces report
    const uint64_t i = cuts[t.order[j]].piece;
    if (c.out_sizes) c.out_sizes[i] = h_osize[j];
    if (c.verdicts) c.verdicts[i] = tab[at.ver + j];
  }
  return LBF_OK;
}

int text_call(const char* who, bool seq, lbf_ctx* ctx, lbf_b64_state* b64_states, lbf_sha1_state* sha_states,
              uint64_t n_states, const uint32_t* state_of, const char* text, uint64_t text_len,
              const uint64_t* text_offsets, const uint32_t* text_lens, const uint8_t* final_flags, uint64_t n,
              const uint32_t* expected_sizes, const uint8_t* expected, uint8_t* out, uint64_t out_len,
              const uint64_t* out_offsets, uint32_t* out_sizes, uint8_t* verdicts) {
  const TextCall call{who,      seq,         b64_states,     sha_states, state_of,
                      reinterpret_cast<const uint8_t*>(text), final_flags,    expected_sizes,
                      expected, out,         out_offsets,    out_sizes,  verdicts};
  return update_call(
      ctx, who, n,
      !b64_states || !sha_states || !text || !text_offsets || !text_lens || !expected_sizes || !out_offsets,
      !out && out_len ? "out is null but out_len is not 0" : nullptr, expected, verdicts, text_offsets, text_lens,
      [&](std::string& why) {
        return seq ? b64_update_seq_check(b64_states, sha_states, n_states, state_of, text_len, text_offsets,
                                          text_lens, final_flags, n, expected_sizes, out_len, out_offsets, why)
                   : b64_update_check(b64_states, sha_states, n_states, state_of, text_len, text_offsets, text_lens, n,
                                      expected_sizes, out_len, out_offsets, why);
      },
      [&](hipStream_t st, const std::vector<UpdateCut>& cuts) { return text_run_launch(ctx, st, call, cuts); });
}

}  // namespace

extern "C" int lbf_sha1_update_batch(lbf_ctx* ctx, lbf_sha1_state* states, uint64_t n_states, const uint32_t* state_of,
                                     const uint8_t* base, uint64_t base_len, const uint64_t* offsets,
                                     const uint32_t* sizes, const uint8_t* final_flags, uint64_t n,
                                     uint8_t* out_digests, const uint8_t* expected, uint8_t* verdicts) {
  return hash_call("lbf_sha1_update_batch", false, ctx, states, n_states, state_of, base, base_len, offsets, sizes,
                   final_flags, n, out_digests, expected, verdicts);
}

extern "C" int lbf_sha1_update_seq_batch(lbf_ctx* ctx, lbf_sha1_state* states, uint64_t n_states,
                                         const uint32_t* state_of, const uint8_t* base, uint64_t base_len,
                                         const uint64_t* offsets, const uint32_t* sizes, const uint8_t* final_flags,
                                         uint64_t n, uint8_t* out_digests, const uint8_t* expected,
                                         uint8_t* verdicts) {
  return hash_call("lbf_sha1_update_seq_batch", true, ctx, states, n_states, state_of, base, base_len, offsets, sizes,
                   final_flags, n, out_digests, expected, verdicts);
}

extern "C" int lbf_b64_update_batch(lbf_ctx* ctx, lbf_b64_state* b64_states, lbf_sha1_state* sha_states,
                                    uint64_t n_states, const uint32_t* state_of, const char* text, uint64_t text_len,
                                    const uint64_t* text_offsets, const uint32_t* text_lens,
                                    const uint8_t* final_flags, uint64_t n, const uint32_t* expected_sizes,
                                    const uint8_t* expected, uint8_t* out, uint64_t out_len,
                                    const uint64_t* out_offsets, uint32_t* out_sizes, uint8_t* verdicts) {
  return text_call("lbf_b64_update_batch", false, ctx, b64_states, sha_states, n_states, state_of, text, text_len,
                   text_offsets, text_lens, final_flags, n, expected_sizes, expected, out, out_len, out_offsets,
                   out_sizes, verdicts);
}

extern "C" int lbf_b64_update_seq_batch(lbf_ctx* ctx, lbf_b64_state* b64_states, lbf_sha1_state* sha_states,
                                        uint64_t n_states, const uint32_t* state_of, const char* text,
                                        uint64_t text_len, const uint64_t* text_offsets, const uint32_t* text_lens,
                                        const uint8_t* final_flags, uint64_t n, const uint32_t* expected_sizes,
                                        const uint8_t* expected, uint8_t* out, uint64_t out_len,
                                        const uint64_t* out_offsets, uint32_t* out_sizes, uint8_t* verdicts) {
  return text_call("lbf_b64_update_seq_batch", true, ctx, b64_states, sha_states, n_states, state_of, text, text_len,
                   text_offsets, text_lens, final_flags, n, expected_sizes, expected, out, out_len, out_offsets,
                   out_sizes, verdicts);
}
