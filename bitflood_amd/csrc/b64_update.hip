// b64_update.hip -- resumable base64 decode on the GPU, chained on the device
// to the resumable SHA-1: one piece of a chunk's text per workgroup, continued
// from a caller-owned 16-byte state (lbf_b64_state, lbf_hash.h).
//
// A SendChunk payload arrives as text, in pieces (ChunkMethods.cpp:137-167).
// The general decode of kern_b64.hpp needs a chunk's whole text; here the
// decoder of xmlrpc++ 0.7 (base64.h:215-330) is stopped between pieces: the
// sextets of an unfinished group are carried in the record, the first '=' ends
// the data for good, and on the final piece an unfinished group is dropped.
// The decoded bytes land in the chunk's slot at their position in the chunk,
// a piece table says where each piece's new bytes lie, and
// lbf_sha1_update_launch absorbs exactly those: the verdict waits only for the
// last piece's share of the chunk.
//
// The kernel here treats a piece as arbitrary text.  The part of a piece that
// continues the encoder's layout is taken first by b64_update_lines.hip's
// kernel (unless lbf_set_b64_lines switched it off), which moves the record on
// and hands over, through the piece table's two arrays, where the chain stood
// and how many characters it took; unbroken text in what that left is taken
// next by b64_flat.hip's kernel (lbf_set_b64_flat), which hands over the same
// two numbers; this kernel decodes what is left.
//
// A translation unit of its own, like sha1_update.hip: the shipped kernels'
// ISA stays as recorded (tests/test_isa.py).  DESIGN.md §4.7.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>

#include <atomic>

#include "b64_flat.hpp"
#include "b64_update_lines.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

struct B64UpdateParams {
  uint8_t* b64_states;          // n_states records of 16 bytes, 16-byte aligned
  uint64_t n_states;
  const uint32_t* state_of;     // chain of each piece, or null: piece i -> chain i
  const uint8_t* text;
  const uint64_t* text_off;
  const uint32_t* text_len;
  const uint8_t* final_flags;   // null => no piece is final
  uint8_t* out;
  const uint64_t* out_off;      // the chunk's slot ...
  const uint32_t* cap;          // ... and its size
  uint32_t* out_sizes;          // written for final pieces only
  uint64_t* piece_off;          // the table lbf_sha1_update_launch reads
  uint32_t* piece_size;
  uint8_t* verdicts;            // the last kernel only
  // the line path ran in front (b64_update_lines.hip): piece_off[i] holds the chain's byte count before the call
  // and piece_size[i] the characters of the piece already decoded; both are overwritten with their final values
  uint32_t lines;
};

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTrip = kThreads * 16;  // characters per trip, as the general decode (kern_b64.hpp)
constexpr uint32_t kMaxCap = 1u << 30;     // the wire calls' bound on a chunk
constexpr uint8_t kEq = 64, kSkip = 255;
// A chain's byte count stays at or below this (the host call refuses a record at
// or past it).  The kernel clamps what it loads to it and a piece adds less than
// 2^32, so no position below ever wraps, whatever a forged record claims.
constexpr uint64_t kMaxDecoded = 1ull << 61;

static_assert(sizeof(lbf_b64_state) == 16 && offsetof(lbf_b64_state, decoded) == 0 &&
                  offsetof(lbf_b64_state, carry) == 8 && offsetof(lbf_b64_state, ncarry) == 12 &&
                  offsetof(lbf_b64_state, ended) == 13 && offsetof(lbf_b64_state, zero) == 14,
              "lbf_b64_state layout");

// The decode table of kern_b64.hpp, restated: that header belongs to
// sha1_kernels.hip's translation unit.
struct Table {
  uint8_t v[256];
};

constexpr Table make_table() {
  Table t{};
  for (int c = 0; c < 256; ++c) t.v[c] = kSkip;
  for (int c = 'A'; c <= 'Z'; ++c) t.v[c] = (uint8_t)(c - 'A');
  for (int c = 'a'; c <= 'z'; ++c) t.v[c] = (uint8_t)(26 + c - 'a');
  for (int c = '0'; c <= '9'; ++c) t.v[c] = (uint8_t)(52 + c - '0');
  t.v['+'] = 62;
  t.v['/'] = 63;
  t.v['='] = kEq;
  return t;
}

__constant__ Table g_update_table = make_table();

// Exclusive scan of one value per lane over the workgroup (wg_exclusive_scan's
// shape, kern_b64.hpp); `sums` is 4 words of LDS.
__device__ __forceinline__ uint32_t scan256(uint32_t v, uint32_t* sums, uint32_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t x = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)x, off, 64);
    if (lane >= off) x += y;
  }
  if (lane == 63) sums[wave] = x;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < (int)kThreads / 64; ++w) {
    const uint32_t s = sums[w];
    before += w < wave ? s : 0u;
    all += s;
  }
  __syncthreads();  // sums is reused by the next trip
  *total = all;
  return before + x - v;
}

// blockIdx.x = piece.  The sextets of a trip go through LDS: sx[0, nc) holds
// the carried sextets, the trip's own follow, so group g of the trip is sx[4g,
// 4g + 4) and a lane's four groups are one aligned 16-byte LDS read.
__global__ void __launch_bounds__(kThreads) b64_update_kernel(B64UpdateParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written (the whole workgroup leaves)
  const uint32_t cap = p.cap[i];
  const bool fin = p.final_flags != nullptr && p.final_flags[i] != 0;
  if (cap > kMaxCap) {  // refused: nothing decoded, nothing for the hash, verdict 0 (b64_length_kernel)
    if (threadIdx.x == 0) {
      p.piece_off[i] = 0;
      p.piece_size[i] = 0;
      if (fin) {
        // the update kernel ends the chain on its empty piece and restarts the SHA record: the pair stays a pair
        p.out_sizes[i] = 0;
        *reinterpret_cast<uint4*>(p.b64_states + 16 * si) = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) uint8_t sx[kTrip + 16];  // 4,096 + 3 sextets, whole 16-byte blocks
  __shared__ uint8_t tab[256];
  __shared__ uint32_t sums[kThreads / 64];
  __shared__ uint32_t first_eq;

  uint8_t* const rec = p.b64_states + 16 * si;
  const uint4 r = *reinterpret_cast<const uint4*>(rec);
  uint64_t decoded = (uint64_t)r.x | ((uint64_t)r.y << 32);
  if (decoded > kMaxDecoded) decoded = kMaxDecoded;  // forged: far past any slot, and it stays there
  // & 3 and the mask: whatever a forged record says, the carry is at most three sextets
  uint32_t nc = r.w & 3u;
  const uint32_t carry = r.z & ((1u << (6u * nc)) - 1u);
  bool ended = ((r.w >> 8) & 0xFFu) != 0;
  uint64_t before = decoded < cap ? decoded : (uint64_t)cap;
  uint32_t taken = 0;
  if (p.lines) {  // the record has moved on by what the line path took: the piece's share starts where it started
    const uint64_t b = p.piece_off[i];
    before = b < cap ? b : (uint64_t)cap;
    taken = p.piece_size[i];
  }

  tab[threadIdx.x] = g_update_table.v[threadIdx.x];
  if (threadIdx.x < 3) sx[threadIdx.x] = (uint8_t)((carry >> (6u * threadIdx.x)) & 63u);
  if (threadIdx.x == 0) first_eq = 0xFFFFFFFFu;
  __syncthreads();

  const uint32_t piece_len = p.text_len[i];
  if (taken > piece_len) taken = piece_len;  // never: the line path takes a prefix
  const uint8_t* const t = p.text + p.text_off[i] + taken;
  const uint64_t len = ended ? 0 : piece_len - taken;
  const uint64_t slot = p.out_off[i];  // positions are sums of 64-bit numbers, taken mod 2^64
  for (uint64_t t0 = 0; t0 < len; t0 += kTrip) {
    // 1. sixteen characters per lane; the ragged end reads as junk
    const uint64_t at = t0 + threadIdx.x * 16u;
    uint8_t c[16];
    if (at + 16 <= len) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(t + at);
      if ((a & 3u) == 0) {
        uint32_t w[4];
        if ((a & 15u) == 0) {
          const uint4 q = *reinterpret_cast<const uint4*>(t + at);
          w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
          const uint32_t* q = reinterpret_cast<const uint32_t*>(t + at);
#pragma unroll
          for (int k = 0; k < 4; ++k) w[k] = q[k];
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) c[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
      } else {
#pragma unroll
        for (int k = 0; k < 16; ++k) c[k] = t[at + k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 16; ++k) c[k] = at + k < len ? t[at + k] : (uint8_t)' ';
    }
    // 2. look up, count; 3. the lane's place among the trip's sextets
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      c[k] = tab[c[k]];
      cnt += c[k] != kSkip;
    }
    uint32_t total;
    uint32_t pos = nc + scan256(cnt, sums, &total);
    // 4. sextets behind the carry; 5. the first '='.  pos < nc + 4,096 <= 4,099
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (c[k] == kSkip) continue;
      if (c[k] == kEq) atomicMin(&first_eq, pos);
      sx[pos++] = c[k];
    }
    __syncthreads();
    // 6. complete groups before any '='
    const uint32_t m = nc + total, feq = first_eq;
    const uint32_t q = feq < m ? feq : m;
    const uint32_t groups = q >> 2, rest = q & 3u;
    // 7. four groups (16 sextets) -> 12 bytes per lane, never at or past cap
    const uint32_t g4 = threadIdx.x * 4u;
    if (g4 < groups) {
      const uint4 v4 = *reinterpret_cast<const uint4*>(sx + 4u * g4);
      const uint32_t vs[4] = {v4.x, v4.y, v4.z, v4.w};
      uint32_t x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t s = vs[k];  // sextets past the complete groups are stale, and their bytes are not written
        x[k] = ((s & 63u) << 18) | (((s >> 8) & 63u) << 12) | (((s >> 16) & 63u) << 6) | ((s >> 24) & 63u);
      }
      uint8_t b[12];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        b[3 * k] = (uint8_t)(x[k] >> 16);
        b[3 * k + 1] = (uint8_t)(x[k] >> 8);
        b[3 * k + 2] = (uint8_t)x[k];
      }
      const uint64_t at_out = decoded + 3ull * g4;  // position in the chunk: at most 2^61 + 3,060, no wrap
      const uint32_t left = groups - g4;
      const uint32_t nb = left >= 4 ? 12u : 3u * left;
      uint8_t* const o = p.out + (slot + at_out);
      if (nb == 12 && cap >= 12u && at_out <= cap - 12u && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(o);
#pragma unroll
        for (int k = 0; k < 3; ++k)
          d[k] = (uint32_t)b[4 * k] | ((uint32_t)b[4 * k + 1] << 8) | ((uint32_t)b[4 * k + 2] << 16) |
                 ((uint32_t)b[4 * k + 3] << 24);
      } else {
        for (uint32_t k = 0; k < nb && at_out + k < cap; ++k) o[k] = b[k];
      }
    }
    const uint64_t at_end = decoded + 3ull * groups;
    if (feq < m) {
      // 8. '=' ends the data: "xx=" gives one more byte, "xxx=" two
      const uint32_t extra = rest == 2 ? 1u : rest == 3 ? 2u : 0u;
      if (threadIdx.x == 0 && extra) {
        const uint32_t a = 4u * groups;
        const uint32_t x = ((uint32_t)sx[a] << 18) | ((uint32_t)sx[a + 1] << 12) |
                           ((uint32_t)(extra == 2 ? sx[a + 2] : 0) << 6);
        uint8_t* const o = p.out + (slot + at_end);
        if (at_end < cap) o[0] = (uint8_t)(x >> 16);
        if (extra == 2 && at_end + 1 < cap) o[1] = (uint8_t)(x >> 8);
      }
      decoded = at_end + extra < kMaxDecoded ? at_end + extra : kMaxDecoded;
      ended = true;
      nc = 0;
      break;  // uniform: feq and m are the same in every lane
    }
    // 9. the unfinished group moves to the front for the next trip
    decoded = at_end < kMaxDecoded ? at_end : kMaxDecoded;
    uint8_t keep = 0;
    if (threadIdx.x < rest) keep = sx[4u * groups + threadIdx.x];
    __syncthreads();  // every read of this trip's sextets is done
    if (threadIdx.x < rest) sx[threadIdx.x] = keep;
    nc = rest;
    // the next trip's barriers (in its scan) come before any lane reads sx again
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const uint64_t after = decoded < cap ? decoded : (uint64_t)cap;
  p.piece_off[i] = slot + before;
  p.piece_size[i] = after > before ? (uint32_t)(after - before) : 0u;  // decoded never falls; checked all the same
  uint4 w = make_uint4(0u, 0u, 0u, 0u);  // as lbf_b64_state_init leaves it: Final() restarts the chain
  if (fin) {
    p.out_sizes[i] = decoded <= cap ? (uint32_t)decoded : cap + 1u;  // an unfinished group is dropped
  } else {
    uint32_t cw = 0;
    for (uint32_t k = 0; k < nc; ++k) cw |= (uint32_t)(sx[k] & 63u) << (6u * k);
    w = make_uint4((uint32_t)decoded, (uint32_t)(decoded >> 32), cw, nc | (ended ? 0x100u : 0u));
  }
  *reinterpret_cast<uint4*>(rec) = w;
}

// A final piece's verdict holds only when its text decoded to the chunk's size
// (ChunkMethods.cpp:156): out_sizes[i] is the decoded length, or cap + 1.
__global__ void __launch_bounds__(256) b64_length_kernel(B64UpdateParams p, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !p.final_flags[i]) return;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;
  const uint32_t cap = p.cap[i];
  if (cap > kMaxCap || p.out_sizes[i] != cap) p.verdicts[i] = 0;
}

}  // namespace

}  // namespace lbf

using lbf::check_fits;
using lbf::fail;

extern "C" void lbf_b64_state_init(lbf_b64_state* states, uint64_t n) {
  if (!states) return;
  for (uint64_t k = 0; k < n; ++k) {
    lbf_b64_state& s = states[k];
    s.decoded = 0;
    s.carry = 0;
    s.ncarry = 0;
    s.ended = 0;
    s.zero = 0;
  }
}

// The line path's switch: LBF_B64_LINES at first use (default on), then lbf_set_b64_lines.
static std::atomic<int> g_b64_lines{-1};

bool lbf::b64_lines_enabled() {
  int v = g_b64_lines.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("LBF_B64_LINES");
    const int from_env = lbf::kB64LinesDefault ? !(e && e[0] == '0' && e[1] == 0) : (e && e[0] == '1' && e[1] == 0);
    g_b64_lines.compare_exchange_strong(v, from_env, std::memory_order_relaxed);  // a setter that got in first wins
    v = g_b64_lines.load(std::memory_order_relaxed);
  }
  return v != 0;
}

extern "C" int lbf_set_b64_lines(int on) {
  const int before = lbf::b64_lines_enabled() ? 1 : 0;
  g_b64_lines.store(on ? 1 : 0, std::memory_order_relaxed);
  return before;
}

extern "C" int lbf_b64_update_launch(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                     const uint32_t* d_state_of, const char* d_text, const uint64_t* d_text_offsets,
                                     const uint32_t* d_text_lens, const uint8_t* d_final, uint64_t n, uint8_t* d_out,
                                     const uint64_t* d_out_offsets, const uint32_t* d_caps, uint32_t* d_out_sizes,
                                     uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                                     uint64_t* d_piece_offsets, uint32_t* d_piece_sizes, void* stream) {
  return lbf::b64_update_launch_counted(d_b64_states, d_sha_states, n_states, d_state_of, d_text, d_text_offsets,
                                        d_text_lens, d_final, n, d_out, d_out_offsets, d_caps, d_out_sizes, d_digests,
                                        d_expected, d_verdicts, d_piece_offsets, d_piece_sizes, nullptr, nullptr,
                                        stream);
}

int lbf::b64_update_launch_counted(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                   const uint32_t* d_state_of, const char* d_text, const uint64_t* d_text_offsets,
                                   const uint32_t* d_text_lens, const uint8_t* d_final, uint64_t n, uint8_t* d_out,
                                   const uint64_t* d_out_offsets, const uint32_t* d_caps, uint32_t* d_out_sizes,
                                   uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                                   uint64_t* d_piece_offsets, uint32_t* d_piece_sizes, uint32_t* d_line_chars,
                                   uint32_t* d_flat_chars, void* stream) {
  const std::string who = "lbf_b64_update_launch";
  if (n == 0) return LBF_OK;
  if (!d_b64_states || !d_sha_states || !d_text || !d_text_offsets || !d_text_lens || !d_out || !d_out_offsets ||
      !d_caps || !d_out_sizes || !d_piece_offsets || !d_piece_sizes)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  // what lbf_sha1_update_launch would refuse is refused here, before the decode is enqueued
  if (d_final && !d_digests && !d_verdicts) return fail(LBF_ERR_INVALID, who + ": no output");
  if ((d_verdicts != nullptr) != (d_expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digest/expected arrays must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_b64_states) & 15u) || (reinterpret_cast<uintptr_t>(d_sha_states) & 15u))
    return fail(LBF_ERR_INVALID, who + ": the state arrays must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_text_offsets) & 7u) || (reinterpret_cast<uintptr_t>(d_out_offsets) & 7u) ||
      (reinterpret_cast<uintptr_t>(d_piece_offsets) & 7u) || (reinterpret_cast<uintptr_t>(d_text_lens) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_caps) & 3u) || (reinterpret_cast<uintptr_t>(d_out_sizes) & 3u) ||
      (reinterpret_cast<uintptr_t>(d_piece_sizes) & 3u) || (reinterpret_cast<uintptr_t>(d_state_of) & 3u))
    return fail(LBF_ERR_INVALID, who + ": a table is not aligned to its element size");
  if (n_states > UINT64_MAX / 96) return fail(LBF_ERR_INVALID, who + ": n_states too large");
  if (int rc = check_fits(d_b64_states, 16 * n_states, "lbf_b64_update_launch: b64_states")) return rc;
  if (int rc = check_fits(d_sha_states, 96 * n_states, "lbf_b64_update_launch: sha_states")) return rc;
  if (int rc = check_fits(d_state_of, 4 * n, "lbf_b64_update_launch: state_of")) return rc;
  if (int rc = check_fits(d_text_offsets, 8 * n, "lbf_b64_update_launch: text_offsets")) return rc;
  if (int rc = check_fits(d_text_lens, 4 * n, "lbf_b64_update_launch: text_lens")) return rc;
  if (int rc = check_fits(d_final, n, "lbf_b64_update_launch: final")) return rc;
  if (int rc = check_fits(d_out_offsets, 8 * n, "lbf_b64_update_launch: out_offsets")) return rc;
  if (int rc = check_fits(d_caps, 4 * n, "lbf_b64_update_launch: caps")) return rc;
  if (int rc = check_fits(d_out_sizes, 4 * n, "lbf_b64_update_launch: out_sizes")) return rc;
  if (int rc = check_fits(d_digests, 20 * n, "lbf_b64_update_launch: digests")) return rc;
  if (int rc = check_fits(d_expected, 20 * n, "lbf_b64_update_launch: expected")) return rc;
  if (int rc = check_fits(d_verdicts, n, "lbf_b64_update_launch: verdicts")) return rc;
  if (int rc = check_fits(d_piece_offsets, 8 * n, "lbf_b64_update_launch: piece_offsets")) return rc;
  if (int rc = check_fits(d_piece_sizes, 4 * n, "lbf_b64_update_launch: piece_sizes")) return rc;
  if (int rc = check_fits(d_line_chars, 4 * n, "lbf_b64_update_launch: line_chars")) return rc;
  if (int rc = check_fits(d_flat_chars, 4 * n, "lbf_b64_update_launch: flat_chars")) return rc;
  lbf::B64UpdateParams p{};
  p.b64_states = reinterpret_cast<uint8_t*>(d_b64_states);
  p.n_states = n_states;
  p.state_of = d_state_of;
  p.text = reinterpret_cast<const uint8_t*>(d_text);
  p.text_off = d_text_offsets;
  p.text_len = d_text_lens;
  p.final_flags = d_final;
  p.out = d_out;
  p.out_off = d_out_offsets;
  p.cap = d_caps;
  p.out_sizes = d_out_sizes;
  p.piece_off = d_piece_offsets;
  p.piece_size = d_piece_sizes;
  p.verdicts = d_verdicts;
  hipStream_t st = (hipStream_t)stream;
  if (lbf::b64_lines_enabled()) {  // the text that continues the encoder's layout, in front of the general rule
    lbf::B64LinesParams lp{};
    lp.b64_states = p.b64_states;
    lp.n_states = n_states;
    lp.state_of = d_state_of;
    lp.text = p.text;
    lp.text_off = d_text_offsets;
    lp.text_len = d_text_lens;
    lp.out = d_out;
    lp.out_off = d_out_offsets;
    lp.cap = d_caps;
    lp.before = d_piece_offsets;
    lp.taken = d_piece_sizes;
    lp.line_chars = d_line_chars;
    if (int rc = lbf::launch_b64_update_lines(lp, (uint32_t)n, st)) return rc;
    p.lines = 1;
  }
  if (lbf::b64_flat_enabled()) {  // unbroken text in what is left: the same hand-over, from or behind the line path's
    lbf::B64FlatParams fp{};
    fp.b64_states = p.b64_states;
    fp.n_states = n_states;
    fp.state_of = d_state_of;
    fp.text = p.text;
    fp.text_off = d_text_offsets;
    fp.text_len = d_text_lens;
    fp.out = d_out;
    fp.out_off = d_out_offsets;
    fp.cap = d_caps;
    fp.before = d_piece_offsets;
    fp.taken = d_piece_sizes;
    fp.flat_chars = d_flat_chars;
    fp.after_lines = p.lines;
    if (int rc = lbf::launch_b64_update_flat(fp, (uint32_t)n, st)) return rc;
    p.lines = 1;
  }
  hipLaunchKernelGGL(lbf::b64_update_kernel, dim3((uint32_t)n), dim3(lbf::kThreads), 0, st, p);
  LBF_HIP_TRY(hipGetLastError());
  if (int rc = lbf_sha1_update_launch(d_sha_states, n_states, d_state_of, d_out, d_piece_offsets, d_piece_sizes,
                                      d_final, n, d_digests, d_expected, d_verdicts, st))
    return rc;
  if (d_final && d_verdicts) {
    hipLaunchKernelGGL(lbf::b64_length_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, p, (uint32_t)n);
    LBF_HIP_TRY(hipGetLastError());
  }
  return LBF_OK;
}
