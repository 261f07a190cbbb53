// update_seq_batch.cpp -- lbf_sha1_update_seq_batch and lbf_b64_update_seq_batch:
// the host batch calls that take several pieces of one state per call and
// absorb them in the caller's order, synchronously on worker 0's first stream.
// What is refused, how a launch's cuts become a chain table and where a chain's
// decoded bytes lie on the device is update_seq_plan.hpp; cutting into launches
// and packing the bytes into copies is update_plan.hpp, as for the calls that
// take one piece per state.  Here the plan meets the stream.  Per launch a
// touched state (pair) travels once, whatever the number of its pieces: the
// device launch names it by chain, and the pieces' tables go up in chain order
// and come back to the caller's piece indices.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "b64_update_seq.hpp"
#include "lbf_host.hpp"
#include "update_seq_plan.hpp"

using namespace lbf;

namespace {

uint64_t up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// The update calls' one allocation on worker 0's device (current when this
// runs), grown on demand; the caller holds ctx->mu.
int seq_scratch(lbf_ctx* ctx, uint64_t need, const char* who) {
  return grow_scratch(ctx->upd_dev, ctx->upd_cap, need, up(need, 1ull << 20), who);
}

// The chain table of one launch's cuts, by the state each cut's piece names.
ChainTable table_of(const std::vector<UpdateCut>& cuts, const uint32_t* state_of) {
  std::vector<uint64_t> ids(cuts.size());
  for (size_t k = 0; k < cuts.size(); ++k) ids[k] = update_state_of(state_of, cuts[k].piece);
  return chain_table(ids);
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

// One launch of the hash call: the chains' states, the tables and the bytes up,
// the kernel, states and results back into the caller's arrays.
int seq_run_launch(lbf_ctx* ctx, hipStream_t st, const UpdateCall& c, const std::vector<UpdateCut>& cuts) {
  const uint64_t m = cuts.size();
  if (m == 0) return LBF_OK;
  std::vector<Run> runs;
  std::vector<uint64_t> dev_off;
  const uint64_t area = update_runs(cuts, runs, dev_off);
  const ChainTable t = table_of(cuts, c.state_of);
  const uint64_t nc = t.chains();
  // inputs: states | offsets | chain_first | sizes | expected | final flags; results: digests | verdicts
  const uint64_t st_b = 96 * nc, off_at = st_b, first_at = off_at + 8 * m, size_at = first_at + 4 * (nc + 1),
                 exp_at = size_at + 4 * m, fin_at = exp_at + 20 * m, in_bytes = fin_at + m;
  std::vector<uint8_t> in(in_bytes, 0), res(21 * m, 0);
  SyncOnExit sync{st};  // after the vectors the copies use: every exit waits for the stream before they go
  lbf_sha1_state* h_states = reinterpret_cast<lbf_sha1_state*>(in.data());
  uint64_t* h_off = reinterpret_cast<uint64_t*>(in.data() + off_at);
  uint32_t* h_size = reinterpret_cast<uint32_t*>(in.data() + size_at);
  for (uint64_t ch = 0; ch < nc; ++ch) h_states[ch] = c.states[t.chain_id[ch]];
  memcpy(in.data() + first_at, t.first.data(), 4 * (nc + 1));
  bool any_final = false;
  for (uint64_t j = 0; j < m; ++j) {  // table position j holds cut order[j]
    const UpdateCut& cut = cuts[t.order[j]];
    h_off[j] = dev_off[t.order[j]];
    h_size[j] = cut.size;
    if (c.expected) memcpy(in.data() + exp_at + 20 * j, c.expected + 20 * cut.piece, 20);
    const bool fin = cut.last && c.final_flags && c.final_flags[cut.piece];
    in[fin_at + j] = fin ? 1 : 0;
    any_final |= fin;
  }
  // device layout: bytes | inputs | results
  const uint64_t data_b = up(area + 16, 256), in_b = up(in_bytes, 256);
  if (int rc = seq_scratch(ctx, data_b + in_b + up(21 * m, 256), "lbf_sha1_update_seq_batch")) return rc;
  uint8_t* d_data = ctx->upd_dev;
  uint8_t* d_in = d_data + data_b;
  uint8_t* d_res = d_in + in_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_data + r.dst, c.base + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_in, in.data(), in.size(), hipMemcpyHostToDevice, st));
  uint8_t* d_dig = d_res;
  uint8_t* d_ver = d_res + 20 * m;
  if (int rc = lbf_sha1_update_seq_launch(
          reinterpret_cast<lbf_sha1_state*>(d_in), nc, nullptr, reinterpret_cast<const uint32_t*>(d_in + first_at), nc,
          d_data, reinterpret_cast<const uint64_t*>(d_in + off_at), reinterpret_cast<const uint32_t*>(d_in + size_at),
          d_in + fin_at, m, d_dig, c.expected ? d_in + exp_at : nullptr, c.expected ? d_ver : nullptr, st))
    return rc;
  LBF_HIP_TRY(hipMemcpyAsync(in.data(), d_in, st_b, hipMemcpyDeviceToHost, st));
  if (any_final) LBF_HIP_TRY(hipMemcpyAsync(res.data(), d_res, res.size(), hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  for (uint64_t ch = 0; ch < nc; ++ch) c.states[t.chain_id[ch]] = h_states[ch];
  for (uint64_t j = 0; j < m; ++j) {
    if (!in[fin_at + j]) continue;  // only final pieces report
    const uint64_t i = cuts[t.order[j]].piece;
    if (c.out_digests) memcpy(c.out_digests + 20 * i, res.data() + 20 * j, 20);
    if (c.verdicts) c.verdicts[i] = res[20 * m + j];
  }
  return LBF_OK;
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

// As b64_update_batch.cpp: below this many bytes per run on average the decoded
// bytes come back as one copy of the launch's area and are scattered on the host.
constexpr uint64_t kDirectRunBytes = 64 << 10;

// One launch of the text call: the chains' state pairs, the tables and the text
// up, the kernels, states and results back into the caller's arrays, then one
// range of decoded bytes per chain.
int seq_text_launch(lbf_ctx* ctx, hipStream_t st, const TextCall& c, const std::vector<UpdateCut>& cuts) {
  const char* who = "lbf_b64_update_seq_batch";
  const uint64_t m = cuts.size();
  if (m == 0) return LBF_OK;
  std::vector<Run> runs, back_runs;
  std::vector<uint64_t> text_off;
  const uint64_t text_area = update_runs(cuts, runs, text_off);
  const ChainTable t = table_of(cuts, c.state_of);
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
  const uint64_t out_area = b64_update_seq_places(decoded, ncarry, chars, cap, places);
  // one block of tables, up and back: b64 states | SHA states (one per chain) | text offsets | slot starts |
  // piece offsets | chain_first | text lengths | chunk sizes | piece sizes | decoded lengths | line-path
  // characters | flat-path characters | expected | digests | final flags | verdicts (one per piece)
  const uint64_t sha_at = 16 * nc, toff_at = sha_at + 96 * nc, slot_at = toff_at + 8 * m, poff_at = slot_at + 8 * m,
                 first_at = poff_at + 8 * m, tlen_at = first_at + 4 * (nc + 1), cap_at = tlen_at + 4 * m,
                 psize_at = cap_at + 4 * m, osize_at = psize_at + 4 * m, lines_at = osize_at + 4 * m,
                 flat_at = lines_at + 4 * m, exp_at = flat_at + 4 * m, dig_at = exp_at + 20 * m,
                 fin_at = dig_at + 20 * m, ver_at = fin_at + m, tab_bytes = ver_at + m;
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
  memcpy(tab.data() + first_at, t.first.data(), 4 * (nc + 1));
  for (uint64_t ch = 0; ch < nc; ++ch) {
    h_b64[ch] = c.b64[t.chain_id[ch]];
    h_sha[ch] = c.sha[t.chain_id[ch]];
    for (uint32_t j = t.first[ch]; j < t.first[ch + 1]; ++j) {  // table position j holds cut order[j]
      const UpdateCut& cut = cuts[t.order[j]];
      h_toff[j] = text_off[t.order[j]];
      h_slot[j] = places[ch].slot;
      h_tlen[j] = cut.size;
      h_cap[j] = cap[ch];
      if (c.expected) memcpy(tab.data() + exp_at + 20 * j, c.expected + 20 * cut.piece, 20);
      tab[fin_at + j] = cut.last && c.final_flags && c.final_flags[cut.piece] ? 1 : 0;
    }
  }
  // device layout: text | decoded bytes | tables
  const uint64_t text_b = up(text_area + 16, 256), out_b = up(out_area + 16, 256);
  if (int rc = seq_scratch(ctx, text_b + out_b + up(tab_bytes, 256), who)) return rc;
  uint8_t* d_text = ctx->upd_dev;
  uint8_t* d_out = d_text + text_b;
  uint8_t* d_tab = d_out + out_b;
  for (const Run& r : runs)
    LBF_HIP_TRY(hipMemcpyAsync(d_text + r.dst, c.text + r.src, r.len, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  if (int rc = b64_update_seq_launch_counted(
          reinterpret_cast<lbf_b64_state*>(d_tab), reinterpret_cast<lbf_sha1_state*>(d_tab + sha_at), nc, nullptr,
          reinterpret_cast<const uint32_t*>(d_tab + first_at), nc, reinterpret_cast<const char*>(d_text),
          reinterpret_cast<const uint64_t*>(d_tab + toff_at), reinterpret_cast<const uint32_t*>(d_tab + tlen_at),
          d_tab + fin_at, m, d_out, reinterpret_cast<const uint64_t*>(d_tab + slot_at),
          reinterpret_cast<const uint32_t*>(d_tab + cap_at), reinterpret_cast<uint32_t*>(d_tab + osize_at),
          d_tab + dig_at, c.expected ? d_tab + exp_at : nullptr, c.expected ? d_tab + ver_at : nullptr,
          reinterpret_cast<uint64_t*>(d_tab + poff_at), reinterpret_cast<uint32_t*>(d_tab + psize_at),
          reinterpret_cast<uint32_t*>(d_tab + lines_at), reinterpret_cast<uint32_t*>(d_tab + flat_at), st))
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
      return fail(LBF_ERR_HIP, std::string(who) + ": a chain decoded past its bound (internal error)");
    got[ch] = (uint32_t)sum;  // at most the chunk's size
    dev_at[ch] = places[ch].dev;
    total += sum;
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
  for (uint64_t ch = 0; ch < nc; ++ch) {
    c.b64[t.chain_id[ch]] = h_b64[ch];
    c.sha[t.chain_id[ch]] = h_sha[ch];
  }
  for (uint64_t j = 0; j < m; ++j) {
    if (!tab[fin_at + j]) continue;  // only final pieces report
    const uint64_t i = cuts[t.order[j]].piece;
    if (c.out_sizes) c.out_sizes[i] = h_osize[j];
    if (c.verdicts) c.verdicts[i] = tab[ver_at + j];
  }
  return LBF_OK;
}

}  // namespace

extern "C" int lbf_sha1_update_seq_batch(lbf_ctx* ctx, lbf_sha1_state* states, uint64_t n_states,
                                         const uint32_t* state_of, const uint8_t* base, uint64_t base_len,
                                         const uint64_t* offsets, const uint32_t* sizes, const uint8_t* final_flags,
                                         uint64_t n, uint8_t* out_digests, const uint8_t* expected,
                                         uint8_t* verdicts) {
  const char* who = "lbf_sha1_update_seq_batch";
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (!states || !base || !offsets || !sizes) return fail(LBF_ERR_INVALID, std::string(who) + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, std::string(who) + ": n too large");
  if ((verdicts != nullptr) != (expected != nullptr))
    return fail(LBF_ERR_INVALID, std::string(who) + ": expected and verdicts go together");
  return guarded([&]() -> int {
    std::string why;
    const uint64_t bad = update_seq_check(states, n_states, state_of, base_len, offsets, sizes, final_flags, n, why);
    if (bad != kNoPiece) return fail(LBF_ERR_INVALID, std::string(who) + ": piece " + std::to_string(bad) + " " + why);
    const std::vector<std::vector<UpdateCut>> launches = update_launches(offsets, sizes, n, ctx->update_bytes);
    const UpdateCall call{states, state_of, base, final_flags, out_digests, expected, verdicts};
    std::lock_guard<std::mutex> lock(ctx->mu);
    KeepCurrentDevice keep;
    Worker& w = ctx->workers[0];
    LBF_HIP_TRY(hipSetDevice(w.device));
    hipStream_t st = w.dev[0].stream;
    for (const std::vector<UpdateCut>& cuts : launches)
      if (int rc = seq_run_launch(ctx, st, call, cuts)) return rc;
    return (int)LBF_OK;
  });
}

extern "C" int lbf_b64_update_seq_batch(lbf_ctx* ctx, lbf_b64_state* b64_states, lbf_sha1_state* sha_states,
                                        uint64_t n_states, const uint32_t* state_of, const char* text,
                                        uint64_t text_len, const uint64_t* text_offsets, const uint32_t* text_lens,
                                        const uint8_t* final_flags, uint64_t n, const uint32_t* expected_sizes,
                                        const uint8_t* expected, uint8_t* out, uint64_t out_len,
                                        const uint64_t* out_offsets, uint32_t* out_sizes, uint8_t* verdicts) {
  const std::string who = "lbf_b64_update_seq_batch";
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
    const uint64_t bad = b64_update_seq_check(b64_states, sha_states, n_states, state_of, text_len, text_offsets,
                                              text_lens, final_flags, n, expected_sizes, out_len, out_offsets, why);
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
      if (int rc = seq_text_launch(ctx, st, call, cuts)) return rc;
    return (int)LBF_OK;
  });
}
