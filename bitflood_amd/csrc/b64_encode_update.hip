// b64_encode_update.hip -- resumable base64 encode on the GPU, beside the
// resumable SHA-1: one piece of a chunk's bytes per workgroup, continued from a
// caller-owned 16-byte state (lbf_b64_enc_state, lbf_hash.h).
//
// The seeder's side of the wire (ChunkMethods.cpp:89-135): the one-shot encode
// of kern_b64.hpp needs a chunk's bytes in one range; here the encoder is
// stopped between pieces.  The one or two bytes of an unfinished group are
// carried in the record; a piece writes the characters of the groups it
// completes at their place in the chunk's text slot -- in xmlrpc++'s lines the
// separators between them too -- and a final piece the last "xx==" / "xxx=".
// The bytes are hashed by lbf_sha1_update_launch, unchanged, in front of the
// encode kernel on the same stream.
//
// The kernel lays tiles of whole lines over the CHUNK's text (not the piece's),
// so that 16-byte text blocks fall at the same places for every cut: a block
// wholly inside the piece's characters is one 16-byte store, the ragged ends go
// byte by byte.  The staging, the block store, the alphabet and a group's
// characters are b64_device.hpp's; the five-word window of a line's block is the
// one-shot encode's (b64_encode_tile, kern_b64.hpp), written out in both: as a
// shared function it changes both kernels' recorded ISA (tests/test_isa.py).
// DESIGN.md §4.8.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "b64_device.hpp"
#include "b64_encode_update.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

using namespace b64e;

static_assert(sizeof(lbf_b64_enc_state) == 16 && offsetof(lbf_b64_enc_state, carry) == 8 &&
                  offsetof(lbf_b64_enc_state, ncarry) == 12 && offsetof(lbf_b64_enc_state, layout) == 13 &&
                  offsetof(lbf_b64_enc_state, zero) == 14,
              "lbf_b64_enc_state layout");

struct EncUpdParams {
  uint8_t* enc_states;         // n_states records of 16 bytes, 16-byte aligned
  uint64_t n_states;
  const uint32_t* state_of;    // chain of each piece, or null: piece i -> chain i
  const uint8_t* base;
  const uint64_t* offsets;
  const uint32_t* sizes;
  const uint8_t* final_flags;  // null => no piece is final
  uint8_t* text;
  const uint64_t* text_off;    // the chunk's text slot ...
  const uint32_t* cap;         // ... and its size
  uint64_t* new_off;
  uint32_t* new_len;           // first the sizes the hash reads (b64_encode_sizes_kernel), then the result
  uint32_t* text_sizes;        // written for final pieces only
  uint8_t* verdicts;           // cleared for a final piece whose text does not fit; may be null
};

// LDS: one block in front of the staged span (the carried bytes go right below
// the piece's first byte), the span's aligned blocks (a tile's bytes at any
// 16-byte phase: one block more than the tile), and slack for the group reads of
// a tile's last window, computed for every word and used only inside the tile.
constexpr uint32_t kFront = 16;
constexpr uint32_t kSpanBlocks = kEncUpdTileBytes / 16 + 1;
constexpr uint32_t kStageBlocks = kSpanBlocks + 3;
constexpr uint32_t kPer = (kSpanBlocks + kEncUpdThreads - 1) / kEncUpdThreads;  // staged blocks per lane
// the last window reads group kEncUpdTileGroups + 4: eight bytes from 3 * that, behind front and phase
static_assert(kFront + 15 + 3 * (kEncUpdTileGroups + 4) + 8 <= 16 * kStageBlocks, "the window stays inside the stage");

// A tile's span (it may be empty), behind the front block.
using EncStage = b64d::Stage<kPer, kEncUpdThreads, kFront / 16>;

// What a piece writes, in 32 bits: the launch's clamps have made everything fit.
struct EncPiece {
  uint8_t* text;     // the slot's first byte
  uint32_t g0, g1;   // the whole groups of the chunk the piece completes: [g0, g1)
  uint32_t partial;  // 1: group g1 is the chunk's last, of `rest` bytes, and a final piece writes it
  uint32_t rest;
  uint32_t lo, hi;   // the text positions written: [lo, hi), hi at most the cap
};

// One tile of the chunk's text from the staged bytes: chunk byte c is LDS byte
// bias + c (mod 2^32).  Lane v writes characters [16v, 16v + 16) of the tile.
// In lines, characters [p, p + 16) of a line lie in at most five consecutive
// "words" of the line's character stream, where word e is group e's four
// characters for e < 18 and, past the line's end, the next line's group e - 18
// shifted one byte right behind the separator; v_alignbyte cuts the block out
// of them.  Unbroken text (kFlat) is the same with the line arithmetic compiled
// out: a block is four groups.  kWhole: every group of the tile is a whole
// group the piece completes, so none needs the range checks; what a window
// computes past the tile comes from stale LDS and is cut away.
template <bool kFlat, bool kWhole>
__device__ __forceinline__ void enc_tile(const uint32_t* w, uint32_t bias, const uint8_t* alpha, uint32_t tile,
                                         const EncPiece& pc) {
  constexpr uint32_t kText = kFlat ? kEncUpdTileFlat : kEncUpdTileText;
  const uint32_t tbeg = tile * kText, gbeg = tile * kEncUpdTileGroups;
  // group gg of the chunk as its four characters, first character in the low byte
  auto chars = [&](uint32_t gg) -> uint32_t {
    if (!kWhole && (gg < pc.g0 || gg >= pc.g1 + pc.partial)) return 0u;  // not this piece's
    const uint32_t x = b64d::group_bits(w, bias + 3 * gg);
    if (kWhole || gg < pc.g1) return b64d::chars_whole(alpha, x);
    return b64d::chars_last(alpha, x, pc.rest);
  };
  for (uint32_t v = threadIdx.x; v < kText / 16; v += kEncUpdThreads) {
    const uint32_t p0 = 16 * v, pos = tbeg + p0;
    if (pos >= pc.hi) break;
    if (pos + 16 <= pc.lo) continue;
    uint4 out;
    if (kFlat) {
      const uint32_t g = gbeg + 4 * v;
      out = make_uint4(chars(g), chars(g + 1), chars(g + 2), chars(g + 3));
    } else {
      const uint32_t line = p0 / kLineChars, col = p0 - kLineChars * line, e0 = col >> 2;
      uint32_t g[5], E[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) g[k] = chars(gbeg + kLineGroups * line + e0 + k);
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        const uint32_t e = e0 + k;
        // past the line's 18 groups: the separator, then the next line's characters one byte right
        E[k] = e <= 17 ? g[k] : (g[k] << 8) | (e == 18 ? (uint32_t)kSeparator : (k > 0 ? g[k - 1] >> 24 : 0u));
      }
      const uint32_t sh = col & 3;
      out = make_uint4(__builtin_amdgcn_alignbyte(E[1], E[0], sh), __builtin_amdgcn_alignbyte(E[2], E[1], sh),
                       __builtin_amdgcn_alignbyte(E[3], E[2], sh), __builtin_amdgcn_alignbyte(E[4], E[3], sh));
    }
    b64d::put_block(pc.text, pos, pc.lo, pc.hi, out);
  }
}

// The sizes the hash reads: the piece's, or none for a piece the encode refuses.
__global__ void __launch_bounds__(256) b64_encode_sizes_kernel(EncUpdParams p, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written for it
  p.new_len[i] = p.cap[i] > kEncMaxTextCap ? 0u : p.sizes[i];
}

// blockIdx.x = piece.  Every branch around a barrier is uniform over the
// workgroup: it depends on the piece's table entries and its chain's record,
// which every lane reads before lane 0 may rewrite it (the first barrier).
__global__ void __launch_bounds__(kEncUpdThreads) b64_encode_update_kernel(EncUpdParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written (the whole workgroup leaves)
  __shared__ uint4 stage[2][kStageBlocks];
  __shared__ uint8_t alpha[64];
  uint8_t* const rec = p.enc_states + 16 * si;
  const uint4 r = *reinterpret_cast<const uint4*>(rec);
  const uint32_t cap = p.cap[i];
  const bool fin = p.final_flags != nullptr && p.final_flags[i] != 0;
  const uint32_t layout = (r.w >> 8) & 1u;
  b64d::fill_alphabet(alpha);
  __syncthreads();
  if (cap > kEncMaxTextCap) {  // refused: nothing encoded, nothing for the hash (b64_encode_sizes_kernel), verdict 0
    if (threadIdx.x == 0) {
      p.new_off[i] = p.text_off[i];
      p.new_len[i] = 0;
      if (fin) {  // the hash ended the chain on its empty piece and restarted its record: the pair stays a pair
        p.text_sizes[i] = 0;
        if (p.verdicts) p.verdicts[i] = 0;
        *reinterpret_cast<uint4*>(rec) = make_uint4(0u, 0u, 0u, layout << 8);
      }
    }
    return;
  }
  // whatever a forged record says: the count stays where no position wraps, the carried bytes are those the count
  // implies, and the layout is one of the two
  uint64_t taken = (uint64_t)r.x | ((uint64_t)r.y << 32);
  if (taken >= kEncMaxTaken) taken = kEncMaxTaken - 1;
  const uint32_t nc = (uint32_t)(taken % 3);
  const uint32_t carry = r.z & ((1u << (8 * nc)) - 1u);
  const bool flat = layout == LBF_B64_LAYOUT_FLAT;
  const uint32_t size = p.sizes[i];
  const uint64_t t1 = taken + size, G0 = taken / 3, G1 = t1 / 3;
  const uint32_t rest = (uint32_t)(t1 % 3);
  const uint64_t P0 = group_pos(G0, flat), Pend = group_pos(G1, flat) + (fin && rest ? 4 : 0);
  const uint64_t lo64 = P0 < cap ? P0 : cap, hi64 = Pend < cap ? Pend : cap;
  const uint8_t* const src = p.base + p.offsets[i];

  if (lo64 < hi64) {  // then P0 < cap: the chain's bytes so far, and every group that starts below the cap, fit 32 bits
    const uint32_t gmax = cap / 4 + 1;  // P(G) >= 4G: a group from here on lies at or past the cap
    EncPiece pc;
    pc.text = p.text + p.text_off[i];
    pc.g0 = (uint32_t)G0;
    pc.g1 = G1 < gmax ? (uint32_t)G1 : gmax;
    pc.partial = fin && rest != 0 && G1 < gmax ? 1u : 0u;
    pc.rest = rest;
    pc.lo = (uint32_t)lo64;
    pc.hi = (uint32_t)hi64;
    const uint32_t t = (uint32_t)taken;
    const uint64_t need = 3ull * pc.g1 + 3;  // the bytes that matter end here
    const uint32_t tend = (uint32_t)(t1 < need ? t1 : need);
    const uint32_t text_tile = flat ? kEncUpdTileFlat : kEncUpdTileText;
    const uint32_t k0 = pc.g0 / kEncUpdTileGroups;
    uint32_t k1 = (pc.g1 + pc.partial - 1) / kEncUpdTileGroups + 1;  // g1 + partial > g0: something is written
    const uint32_t kcap = (pc.hi - 1) / text_tile + 1;
    if (k1 > kcap) k1 = kcap;

    EncStage st;
    uint32_t cbeg = 0;  // the chunk byte the staged span starts at
    auto load = [&](uint32_t tile) {
      const uint32_t tb = tile * kEncUpdTileBytes, te = tb + kEncUpdTileBytes;
      cbeg = tb > t ? tb : t;
      const uint32_t cend = te < tend ? te : tend;
      const uint32_t len = cend > cbeg ? cend - cbeg : 0u;
      st.clear();
      if (len != 0) st.load(src + (cbeg - t), len);
    };
    load(k0);  // k0's tile starts at or below 3 * g0 <= t: its span starts at the piece's first byte
    st.store(stage[0]);
    uint32_t bias = kFront + st.delta - cbeg;
    if (threadIdx.x == 0) {
      // the carried group: its first nc bytes right below the piece's first (lane 0 stored that block itself)
      uint8_t* sb = reinterpret_cast<uint8_t*>(stage[0]);
      for (uint32_t k = 0; k < nc; ++k) sb[kFront + st.delta - nc + k] = (uint8_t)(carry >> (8 * k));
    }
    __syncthreads();
    for (uint32_t tile = k0; tile < k1; ++tile) {
      const uint32_t buf = (tile - k0) & 1u;
      if (tile + 1 < k1) load(tile + 1);  // in flight while this tile encodes
      const uint32_t* w = reinterpret_cast<const uint32_t*>(stage[buf]);
      const bool whole = tile * kEncUpdTileGroups >= pc.g0 && (tile + 1) * kEncUpdTileGroups <= pc.g1;
      if (flat) {
        if (whole) enc_tile<true, true>(w, bias, alpha, tile, pc);
        else enc_tile<true, false>(w, bias, alpha, tile, pc);
      } else {
        if (whole) enc_tile<false, true>(w, bias, alpha, tile, pc);
        else enc_tile<false, false>(w, bias, alpha, tile, pc);
      }
      if (tile + 1 < k1) {
        st.store(stage[buf ^ 1u]);
        bias = kFront + st.delta - cbeg;
        __syncthreads();
      }
    }
  }

  if (threadIdx.x != 0) return;
  // the record moves on: the bytes of the unfinished group, from the piece or, for a piece shorter than that, from
  // what was carried
  const uint32_t nr = fin ? 0u : rest;
  uint32_t ncarry = 0;
  for (uint32_t k = 0; k < nr; ++k) {
    const uint64_t c = t1 - nr + k;  // chunk byte
    const uint32_t b = c >= taken ? (uint32_t)src[c - taken] : (carry >> (8 * (uint32_t)(c - (taken - nc)))) & 255u;
    ncarry |= b << (8 * k);
  }
  const uint64_t now = fin ? 0ull : t1;
  *reinterpret_cast<uint4*>(rec) = make_uint4((uint32_t)now, (uint32_t)(now >> 32), ncarry, nr | layout << 8);
  p.new_off[i] = p.text_off[i] + lo64;
  p.new_len[i] = (uint32_t)(hi64 - lo64);
  if (fin) {
    const bool fits = Pend <= cap;
    p.text_sizes[i] = fits ? (uint32_t)Pend : cap + 1;
    if (!fits && p.verdicts) p.verdicts[i] = 0;  // behind the hash on the stream: its verdict does not stand
  }
}

}  // namespace

}  // namespace lbf

using lbf::check_fits;
using lbf::fail;

extern "C" void lbf_b64_enc_state_init(lbf_b64_enc_state* states, uint64_t n, int layout) {
  if (!states) return;
  for (uint64_t k = 0; k < n; ++k) {
    lbf_b64_enc_state& s = states[k];
    s.taken = 0;
    s.carry = 0;
    s.ncarry = 0;
    s.layout = layout == LBF_B64_LAYOUT_FLAT ? LBF_B64_LAYOUT_FLAT : LBF_B64_LAYOUT_XMLRPC;
    s.zero = 0;
  }
}

extern "C" uint64_t lbf_b64_text_length(uint64_t size, int layout) {
  return lbf::b64e::text_length(size, layout == LBF_B64_LAYOUT_FLAT);
}

extern "C" int lbf_b64_encode_update_launch(lbf_b64_enc_state* d_enc_states, lbf_sha1_state* d_sha_states,
                                            uint64_t n_states, const uint32_t* d_state_of, const uint8_t* d_base,
                                            const uint64_t* d_offsets, const uint32_t* d_sizes, const uint8_t* d_final,
                                            uint64_t n, char* d_text, const uint64_t* d_text_offsets,
                                            const uint32_t* d_text_caps, uint64_t* d_new_offsets, uint32_t* d_new_lens,
                                            uint32_t* d_text_sizes, uint8_t* d_digests, const uint8_t* d_expected,
                                            uint8_t* d_verdicts, void* stream) {
  const std::string who = "lbf_b64_encode_update_launch";
  if (n == 0) return LBF_OK;
  if (!d_enc_states || !d_sha_states || !d_base || !d_offsets || !d_sizes || !d_text || !d_text_offsets ||
      !d_text_caps || !d_new_offsets || !d_new_lens || !d_text_sizes)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  // what lbf_sha1_update_launch would refuse is refused here, before anything is enqueued
  if (d_final && !d_digests && !d_verdicts) return fail(LBF_ERR_INVALID, who + ": no output");
  if ((d_verdicts != nullptr) != (d_expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digest/expected arrays must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_enc_states) & 15u) || (reinterpret_cast<uintptr_t>(d_sha_states) & 15u))
    return fail(LBF_ERR_INVALID, who + ": the state arrays must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_offsets) & 7u) || (reinterpret_cast<uintptr_t>(d_text_offsets) & 7u) ||
      (reinterpret_cast<uintptr_t>(d_new_offsets) & 7u) || (reinterpret_cast<uintptr_t>(d_sizes) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_text_caps) & 3u) || (reinterpret_cast<uintptr_t>(d_new_lens) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_text_sizes) & 3u) || (reinterpret_cast<uintptr_t>(d_state_of) & 3u))
    return fail(LBF_ERR_INVALID, who + ": a table is not aligned to its element size");
  if (n_states > UINT64_MAX / 96) return fail(LBF_ERR_INVALID, who + ": n_states too large");
  if (int rc = check_fits(d_enc_states, 16 * n_states, "lbf_b64_encode_update_launch: enc_states")) return rc;
  if (int rc = check_fits(d_sha_states, 96 * n_states, "lbf_b64_encode_update_launch: sha_states")) return rc;
  if (int rc = check_fits(d_state_of, 4 * n, "lbf_b64_encode_update_launch: state_of")) return rc;
  if (int rc = check_fits(d_offsets, 8 * n, "lbf_b64_encode_update_launch: offsets")) return rc;
  if (int rc = check_fits(d_sizes, 4 * n, "lbf_b64_encode_update_launch: sizes")) return rc;
  if (int rc = check_fits(d_final, n, "lbf_b64_encode_update_launch: final")) return rc;
  if (int rc = check_fits(d_text_offsets, 8 * n, "lbf_b64_encode_update_launch: text_offsets")) return rc;
  if (int rc = check_fits(d_text_caps, 4 * n, "lbf_b64_encode_update_launch: text_caps")) return rc;
  if (int rc = check_fits(d_new_offsets, 8 * n, "lbf_b64_encode_update_launch: new_offsets")) return rc;
  if (int rc = check_fits(d_new_lens, 4 * n, "lbf_b64_encode_update_launch: new_lens")) return rc;
  if (int rc = check_fits(d_text_sizes, 4 * n, "lbf_b64_encode_update_launch: text_sizes")) return rc;
  if (int rc = check_fits(d_digests, 20 * n, "lbf_b64_encode_update_launch: digests")) return rc;
  if (int rc = check_fits(d_expected, 20 * n, "lbf_b64_encode_update_launch: expected")) return rc;
  if (int rc = check_fits(d_verdicts, n, "lbf_b64_encode_update_launch: verdicts")) return rc;
  lbf::EncUpdParams p{};
  p.enc_states = reinterpret_cast<uint8_t*>(d_enc_states);
  p.n_states = n_states;
  p.state_of = d_state_of;
  p.base = d_base;
  p.offsets = d_offsets;
  p.sizes = d_sizes;
  p.final_flags = d_final;
  p.text = reinterpret_cast<uint8_t*>(d_text);
  p.text_off = d_text_offsets;
  p.cap = d_text_caps;
  p.new_off = d_new_offsets;
  p.new_len = d_new_lens;
  p.text_sizes = d_text_sizes;
  p.verdicts = d_verdicts;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lbf::b64_encode_sizes_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, p,
                     (uint32_t)n);
  LBF_HIP_TRY(hipGetLastError());
  if (int rc = lbf_sha1_update_launch(d_sha_states, n_states, d_state_of, d_base, d_offsets, d_new_lens, d_final, n,
                                      d_digests, d_expected, d_verdicts, st))
    return rc;
  hipLaunchKernelGGL(lbf::b64_encode_update_kernel, dim3((uint32_t)n), dim3(lbf::b64e::kEncUpdThreads), 0, st, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}
