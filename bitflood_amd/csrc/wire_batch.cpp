// wire_batch.cpp -- the two batch calls of the wire (base64) form: chunks to
// send are verified and encoded, received chunks are decoded and verified, on
// the device, synchronously on worker 0's first stream.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>

#include "b64_flat.hpp"
#include "b64_flat_encode.hpp"
#include "lbf_host.hpp"

using namespace lbf;

namespace {

// The device memory of the two base64 entry points: one allocation on worker
// 0's device (current when this runs), grown on demand; the caller holds ctx->mu.
int b64_scratch(lbf_ctx* ctx, uint64_t need, const char* who) {
  return grow_scratch(ctx->b64_dev, ctx->b64_cap, need, std::max<uint64_t>(need, 64ull << 20), who);
}

// The runs of caller slots a D2H writes (stage_plan.hpp, slot_runs).
int checked_slot_runs(const uint64_t* off, const uint64_t* len, uint64_t n, const char* who,
                      std::vector<SlotRun>& runs) {
  const uint64_t bad = slot_runs(off, len, n, runs);
  if (bad == kNoSlot) return LBF_OK;
  return fail(LBF_ERR_INVALID, std::string(who) + ": slot " + std::to_string(bad) + " overlaps another slot");
}

// The wire kernels keep text and byte positions inside a chunk, and their
// tile counts, in 32 bits (kern_b64.hpp): (len + tile - 1) / tile and
// tile * tile_text must not wrap, so chunks are bounded well below 2^32.  The
// reference's chunks are 64 KiB to a few MiB (Encoder.cpp:17-102); 1 GiB of
// bytes encodes to 1.43 GB of text.  ADVICE r05: past 2^32 the positions
// wrapped and tiles were never launched.
constexpr uint64_t kB64MaxText = 3ull << 29;

}  // namespace

extern "C" uint64_t lbf_b64_put_length(uint64_t size) { return b64e::text_length(size, false); }

namespace {

// Chunks to send: verify on the device (ChunkMethods.cpp:116-123), then encode
// each as the base64 text of its SendChunk frame from the same device copy, in
// xmlrpc++'s lines (XmlRpcValue.cpp:439-452, kern_b64.hpp) or unbroken, as the
// Java and Perl peers write it (b64_flat_encode.hip).  Synchronous on worker
// 0's first stream: one H2D of the bytes' span and one of the tables, two
// launches, one D2H of the verdicts and one per run of text slots.  `who` names
// the entry point in the refusals.
int verify_encode_b64(lbf_ctx* ctx, const uint8_t* data, uint64_t data_len, const uint64_t* offsets,
                      const uint32_t* sizes, uint64_t n, const uint8_t* expected, uint8_t* verdicts, int layout,
                      char* text, uint64_t text_len, const uint64_t* text_offsets, const std::string& who) {
  if (int rc = check_b64_layout(who, layout)) return rc;
  if (n != 0 && (!data || !offsets || !sizes || !expected || !verdicts || !text || !text_offsets))
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n too large");
  uint64_t dlo = UINT64_MAX, dhi = 0, tlo = UINT64_MAX, thi = 0;
  std::vector<uint64_t> tlens(n);
  uint32_t max_size = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (sizes[i] > b64e::kEncMaxChunk)
      return fail(LBF_ERR_INVALID, who + ": chunk " + std::to_string(i) + " larger than the wire encode takes (1 GiB)");
    if (offsets[i] > data_len || sizes[i] > data_len - offsets[i])
      return fail(LBF_ERR_INVALID, who + ": chunk " + std::to_string(i) + " outside the buffer");
    const uint64_t tl = tlens[i] = lbf_b64_text_length(sizes[i], layout);
    if (text_offsets[i] > text_len || tl > text_len - text_offsets[i])
      return fail(LBF_ERR_INVALID, who + ": text slot " + std::to_string(i) + " outside the buffer");
    dlo = std::min(dlo, offsets[i]);
    dhi = std::max(dhi, offsets[i] + sizes[i]);
    tlo = std::min(tlo, text_offsets[i]);
    thi = std::max(thi, text_offsets[i] + tl);
    max_size = std::max(max_size, sizes[i]);
  }
  std::vector<SlotRun> runs;  // the text slots the D2H writes, and nothing between them
  if (int rc = checked_slot_runs(text_offsets, tlens.data(), n, who.c_str(), runs)) return rc;
  dlo &= ~15ull;  // device offsets keep the host offsets' alignment mod 16
  tlo &= ~15ull;
  return guarded([&] {
    std::vector<uint8_t> in(n * (8 + 8 + 4 + 20));
    uint64_t* doff = reinterpret_cast<uint64_t*>(in.data());
    uint64_t* toff = doff + n;
    uint32_t* sz = reinterpret_cast<uint32_t*>(toff + n);
    for (uint64_t i = 0; i < n; ++i) {
      doff[i] = offsets[i] - dlo;
      toff[i] = text_offsets[i] - tlo;
      sz[i] = sizes[i];
    }
    memcpy(sz + n, expected, 20 * n);
    // device layout: bytes | text | inputs (offsets, text offsets, sizes, expected) | verdicts
    const uint64_t data_b = round_up(dhi - dlo + 16, 256), text_b = round_up(thi - tlo + 16, 256);
    const uint64_t in_b = round_up(in.size(), 256);
    const uint64_t need = data_b + text_b + in_b + round_up(n, 256);
    std::lock_guard<std::mutex> lock(ctx->mu);
    KeepCurrentDevice keep;
    Worker& w = ctx->workers[0];
    LBF_HIP_TRY(hipSetDevice(w.device));
    if (int rc = b64_scratch(ctx, need, who.c_str())) return rc;
    uint8_t* d_data = ctx->b64_dev;
    uint8_t* d_text = d_data + data_b;
    uint8_t* d_in = d_text + text_b;
    uint8_t* d_ver = d_in + in_b;
    hipStream_t st = w.dev[0].stream;
    SyncOnExit sync{st};
    if (dhi > dlo) LBF_HIP_TRY(hipMemcpyAsync(d_data, data + dlo, dhi - dlo, hipMemcpyHostToDevice, st));
    LBF_HIP_TRY(hipMemcpyAsync(d_in, in.data(), in.size(), hipMemcpyHostToDevice, st));
    const uint64_t* d_doff = reinterpret_cast<const uint64_t*>(d_in);
    const uint64_t* d_toff = d_doff + n;
    const uint32_t* d_sz = reinterpret_cast<const uint32_t*>(d_toff + n);
    const uint8_t* d_exp = reinterpret_cast<const uint8_t*>(d_sz + n);
    if (int rc = lbf_sha1_launch(d_data, d_doff, d_sz, n, nullptr, d_exp, d_ver, st)) return rc;
    if (int rc = launch_b64_encode_for(layout, d_data, d_doff, d_sz, d_text, d_toff, (uint32_t)n, max_size, st))
      return rc;
    LBF_HIP_TRY(hipMemcpyAsync(verdicts, d_ver, n, hipMemcpyDeviceToHost, st));
    for (const SlotRun& r : runs)
      LBF_HIP_TRY(hipMemcpyAsync(text + r.lo, d_text + (r.lo - tlo), r.hi - r.lo, hipMemcpyDeviceToHost, st));
    LBF_HIP_TRY(hipStreamSynchronize(st));
    return (int)LBF_OK;
  });
}

}  // namespace

extern "C" int lbf_verify_encode_b64_batch(lbf_ctx* ctx, const uint8_t* data, uint64_t data_len,
                                           const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                                           const uint8_t* expected, uint8_t* verdicts, char* text, uint64_t text_len,
                                           const uint64_t* text_offsets) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");  // this call's first refusal, as it has always been
  return verify_encode_b64(ctx, data, data_len, offsets, sizes, n, expected, verdicts, LBF_B64_LAYOUT_XMLRPC, text,
                           text_len, text_offsets, "lbf_verify_encode_b64_batch");
}

extern "C" int lbf_verify_encode_b64_layout_batch(lbf_ctx* ctx, const uint8_t* data, uint64_t data_len,
                                                  const uint64_t* offsets, const uint32_t* sizes, uint64_t n,
                                                  const uint8_t* expected, uint8_t* verdicts, int layout, char* text,
                                                  uint64_t text_len, const uint64_t* text_offsets) {
  return verify_encode_b64(ctx, data, data_len, offsets, sizes, n, expected, verdicts, layout, text, text_len,
                           text_offsets, "lbf_verify_encode_b64_layout_batch");
}

namespace {

// One lbf_b64_verify_batch call: the caller's arguments, and what the checks
// derive from them.
struct B64Verify {
  const char* text;
  const uint64_t* text_offsets;
  const uint32_t* text_lens;
  uint64_t n;
  const uint32_t* expected_sizes;
  const uint8_t* expected;
  uint8_t* out;
  const uint64_t* out_offsets;
  uint32_t* out_sizes;
  uint8_t* verdicts;
  uint64_t tlo = UINT64_MAX, thi = 0, olo = UINT64_MAX, ohi = 0;  // the spans of the text and of the output slots
  uint32_t max_tlen = 0, max_cap = 0;  // of the chunks the one-pass decode gets
  std::vector<SlotRun> runs;  // the output slots the D2H writes, and nothing between them
  // The chunks' order on the device: order[k] = the caller's index of device chunk k.  The first n_canon go
  // through the one-pass decode; the rest are the flat pass's candidates (b64_flat.hpp), which skip it -- their
  // text would fail it at the first separator place.  With the flat path off: the caller's order, n_canon = n.
  std::vector<uint32_t> order;
  uint64_t n_canon = 0;
  uint32_t flat_tlen = 0;  // the candidates' longest text
  // bytes per chunk of the inputs (offsets, lengths, caps, expected) and of the results (sizes, over,
  // verdicts, redo flags); kIn * n keeps 4-byte alignment
  static constexpr uint64_t kIn = 8 * 3 + 4 * 2 + 20, kRes = 4 + 1 + 1 + 1;
};

int b64_verify_check(B64Verify& v, uint64_t text_len, uint64_t out_len) {
  const uint64_t n = v.n;
  for (uint64_t i = 0; i < n; ++i) {
    if (v.text_lens[i] > kB64MaxText || v.expected_sizes[i] > b64e::kEncMaxChunk)
      return fail(LBF_ERR_INVALID, "lbf_b64_verify_batch: chunk " + std::to_string(i) +
                                       " larger than the wire decode takes (1 GiB of bytes, 1.5 GiB of text)");
    if (v.text_offsets[i] > text_len || v.text_lens[i] > text_len - v.text_offsets[i])
      return fail(LBF_ERR_INVALID, "lbf_b64_verify_batch: text range " + std::to_string(i) + " outside the buffer");
    v.tlo = std::min(v.tlo, v.text_offsets[i]);
    v.thi = std::max(v.thi, v.text_offsets[i] + v.text_lens[i]);
    if (v.out) {
      if (v.out_offsets[i] > out_len || v.expected_sizes[i] > out_len - v.out_offsets[i])
        return fail(LBF_ERR_INVALID, "lbf_b64_verify_batch: output slot " + std::to_string(i) + " outside the buffer");
      v.olo = std::min(v.olo, v.out_offsets[i]);
      v.ohi = std::max(v.ohi, v.out_offsets[i] + v.expected_sizes[i]);
    }
  }
  // device offsets keep the host offsets' alignment mod 16; the D2H writes the
  // output slots and nothing between them
  if (v.out) {
    std::vector<uint64_t> olens(v.expected_sizes, v.expected_sizes + n);
    if (int rc = checked_slot_runs(v.out_offsets, olens.data(), n, "lbf_b64_verify_batch", v.runs)) return rc;
  }
  const bool flat = b64_flat_enabled();
  v.order.reserve(n);
  std::vector<uint32_t> candidates;
  for (uint64_t i = 0; i < n; ++i) {
    if (flat && b64_flat_candidate(v.text_lens[i], v.expected_sizes[i])) {
      candidates.push_back((uint32_t)i);
      v.flat_tlen = std::max(v.flat_tlen, v.text_lens[i]);
      continue;
    }
    v.order.push_back((uint32_t)i);
    v.max_tlen = std::max(v.max_tlen, v.text_lens[i]);
    v.max_cap = std::max(v.max_cap, v.expected_sizes[i]);
  }
  v.n_canon = v.order.size();
  v.order.insert(v.order.end(), candidates.begin(), candidates.end());
  v.tlo &= ~15ull;
  if (v.out) v.olo &= ~15ull;
  return LBF_OK;
}

// The upload of one call: the inputs and, right behind them, the zeroed
// results, so one H2D carries both and one D2H brings the results back.
// Returns the bytes of sextet scratch and of decoded output the device needs.
std::vector<uint8_t> b64_verify_tables(const B64Verify& v, uint64_t& sext, uint64_t& outb) {
  const uint64_t n = v.n;
  std::vector<uint64_t> toff(n), soff(n), ooff(n);
  std::vector<uint32_t> tlen(n), cap(n);
  sext = 0, outb = 0;
  std::vector<uint8_t> exp(20 * n);
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = v.order[k];
    toff[k] = v.text_offsets[i] - v.tlo;
    soff[k] = sext;
    sext += round_up(v.text_lens[i], 16);
    tlen[k] = v.text_lens[i];
    cap[k] = v.expected_sizes[i];
    memcpy(exp.data() + 20 * k, v.expected + 20 * i, 20);
    if (v.out) {
      ooff[k] = v.out_offsets[i] - v.olo;
    } else {
      ooff[k] = outb;
      outb += round_up(v.expected_sizes[i], 16);
    }
  }
  if (v.out) outb = v.ohi - v.olo;
  std::vector<uint8_t> in(n * (B64Verify::kIn + B64Verify::kRes), 0);
  uint8_t* q = in.data();
  auto put = [&](const void* src, uint64_t bytes) {
    memcpy(q, src, bytes);
    q += bytes;
  };
  put(toff.data(), 8 * n);
  put(soff.data(), 8 * n);
  put(ooff.data(), 8 * n);
  put(tlen.data(), 4 * n);
  put(cap.data(), 4 * n);
  put(exp.data(), 20 * n);
  return in;
}

// The results of one call (sizes, over, verdicts, redo flags per chunk, in the
// device's order) as the caller's verdicts and sizes, and the context's
// decode-path counters.  A candidate of the flat pass is "not the encoder's
// layout" whichever kernel decoded it: general_chunks counts it, and
// flat_chunks those of them the flat pass kept.
void b64_verify_results(lbf_ctx* ctx, const B64Verify& v, const std::vector<uint8_t>& res) {
  const uint64_t n = v.n;
  const uint8_t* redo = res.data() + 6 * n;
  uint64_t general = n - v.n_canon, flat = 0;
  for (uint64_t k = 0; k < v.n_canon; ++k) general += redo[k] != 0;
  for (uint64_t k = v.n_canon; k < n; ++k) flat += redo[k] == 0;
  ctx->b64_general += general;
  ctx->b64_one_pass += n - general;
  ctx->b64_flat_chunks += flat;
  const uint32_t* sizes = reinterpret_cast<const uint32_t*>(res.data());
  const uint8_t* over = res.data() + 4 * n;
  const uint8_t* ver = over + n;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = v.order[k];
    // ChunkMethods.cpp:156: the decoded length must be the chunk's size
    const bool longer = over[k] != 0;
    v.verdicts[i] = (ver[k] && !longer && sizes[k] == v.expected_sizes[i]) ? 1 : 0;
    if (v.out_sizes) v.out_sizes[i] = longer ? v.expected_sizes[i] + 1 : sizes[k];
  }
}

int b64_verify_run(lbf_ctx* ctx, const B64Verify& v) {
  const uint64_t n = v.n, kIn = B64Verify::kIn, kRes = B64Verify::kRes;
  uint64_t sext = 0, outb = 0;
  const std::vector<uint8_t> in = b64_verify_tables(v, sext, outb);
  // device layout: text | sextets | bytes | inputs then, right behind them, the results
  const uint64_t text_b = round_up(v.thi - v.tlo, 256), sext_b = round_up(sext, 256), out_b = round_up(outb + 16, 256);
  const uint64_t io_b = round_up(n * (kIn + kRes), 256);
  const uint64_t need = text_b + sext_b + out_b + io_b;
  std::lock_guard<std::mutex> lock(ctx->mu);
  KeepCurrentDevice keep;
  Worker& w = ctx->workers[0];
  LBF_HIP_TRY(hipSetDevice(w.device));
  if (int rc = b64_scratch(ctx, need, "lbf_b64_verify_batch")) return rc;
  uint8_t* d_text = ctx->b64_dev;
  uint8_t* d_sext = d_text + text_b;
  uint8_t* d_out = d_sext + sext_b;
  uint8_t* d_in = d_out + out_b;
  uint8_t* d_res = d_in + kIn * n;
  hipStream_t st = w.dev[0].stream;
  std::vector<uint8_t> res(n * kRes);
  SyncOnExit sync{st};
  if (v.thi > v.tlo) LBF_HIP_TRY(hipMemcpyAsync(d_text, v.text + v.tlo, v.thi - v.tlo, hipMemcpyHostToDevice, st));
  LBF_HIP_TRY(hipMemcpyAsync(d_in, in.data(), in.size(), hipMemcpyHostToDevice, st));
  const uint64_t* d_toff = reinterpret_cast<const uint64_t*>(d_in);
  const uint64_t* d_soff = d_toff + n;
  const uint64_t* d_ooff = d_soff + n;
  const uint32_t* d_tlen = reinterpret_cast<const uint32_t*>(d_ooff + n);
  const uint32_t* d_cap = d_tlen + n;
  const uint8_t* d_exp = reinterpret_cast<const uint8_t*>(d_cap + n);
  uint32_t* d_sizes = reinterpret_cast<uint32_t*>(d_res);
  uint8_t* d_over = reinterpret_cast<uint8_t*>(d_sizes + n);
  uint8_t* d_ver = d_over + n;
  uint8_t* d_redo = d_ver + n;  // uploaded as zeros
  lbf::B64Launch b{d_text, d_sext, d_toff, d_soff, d_tlen, d_out,   d_ooff, d_cap,
                   d_sizes, d_over, d_redo, (uint32_t)n, v.max_tlen, v.max_cap};
  // the one-pass decode of the first n_canon chunks, the flat pass of the candidates behind them, then the
  // general decode of whatever either handed back
  lbf::B64Launch canon = b;
  canon.n = (uint32_t)v.n_canon;
  if (int rc = lbf::launch_b64_decode_one_pass(canon, st)) return rc;
  if (v.n_canon < n) {
    const lbf::B64FlatDecode f{d_text, d_toff, d_tlen, d_out, d_ooff, d_cap, d_sizes, d_over, d_redo,
                               (uint32_t)v.n_canon, (uint32_t)(n - v.n_canon), v.flat_tlen};
    if (int rc = lbf::launch_b64_flat_decode(f, st)) return rc;
  }
  if (int rc = lbf::launch_b64_decode_general(b, st)) return rc;
  // the decoded lengths are the chunk sizes the hash kernels read
  if (int rc = lbf_sha1_launch(d_out, d_ooff, d_sizes, n, nullptr, d_exp, d_ver, st)) return rc;
  LBF_HIP_TRY(hipMemcpyAsync(res.data(), d_res, res.size(), hipMemcpyDeviceToHost, st));
  for (const SlotRun& r : v.runs)
    LBF_HIP_TRY(hipMemcpyAsync(v.out + r.lo, d_out + (r.lo - v.olo), r.hi - r.lo, hipMemcpyDeviceToHost, st));
  LBF_HIP_TRY(hipStreamSynchronize(st));
  b64_verify_results(ctx, v, res);
  return LBF_OK;
}

}  // namespace

// Received chunks as base64 text: decode on the device (kern_b64.hpp), then
// the shipped hash kernels verify the decoded bytes in HBM.  Synchronous on
// worker 0's first stream: one H2D of the text span and one of the tables, two
// launches, one D2H of the results and one of the decoded span.
extern "C" int lbf_b64_verify_batch(lbf_ctx* ctx, const char* text, uint64_t text_len,
                                    const uint64_t* text_offsets, const uint32_t* text_lens, uint64_t n,
                                    const uint32_t* expected_sizes, const uint8_t* expected, uint8_t* out,
                                    uint64_t out_len, const uint64_t* out_offsets, uint32_t* out_sizes,
                                    uint8_t* verdicts) {
  if (!ctx) return fail(LBF_ERR_INVALID, "null context");
  if (n == 0) return LBF_OK;
  if (!text || !text_offsets || !text_lens || !expected_sizes || !expected || !verdicts)
    return fail(LBF_ERR_INVALID, "lbf_b64_verify_batch: null argument");
  if (out && !out_offsets) return fail(LBF_ERR_INVALID, "lbf_b64_verify_batch: out without out_offsets");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, "lbf_b64_verify_batch: n too large");
  return guarded([&] {
    B64Verify v{text, text_offsets, text_lens, n, expected_sizes, expected, out, out_offsets, out_sizes, verdicts};
    if (int rc = b64_verify_check(v, text_len, out_len)) return rc;
    return b64_verify_run(ctx, v);
  });
}
