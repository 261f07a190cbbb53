// b64_flat.hip -- the flat path of the base64 decode: unbroken RFC 4648 text,
// 4 * ceil(size / 3) characters with '=' padding and nothing else.
//
// bitflood's three peers do not lay a chunk's base64 out the same way.
// xmlrpc++ (C++) writes lines of 72 alphabet characters and a separator, and
// kern_b64.hpp's one-pass decode and b64_update_lines.hip place every
// character by that layout.  The Java peer sends Base64.encodeToString(arg,
// false) (java/com/net/BitFlood/XMLEnvelopeProcessor.java:124, sdk/Base64.java
// with lineSep == false) and the Perl peer MIME::Base64::encode_base64($value,
// '') (perl/RPC/XML.pm:638, :671, :734): no separators at all.  For such a
// text character i is sextet i: group g is characters [4g, 4g + 4) and bytes
// [3g, 3g + 3), with no columns and no separator places.  Two kernels:
//
//   b64_flat_decode_kernel   the one-shot pass of lbf_b64_verify_batch, for
//       chunks whose text length is the unbroken text's and not the encoder's.
//       The one-pass decode's shape (kern_b64.hpp): tiles of 3,888 bytes = 243
//       blocks of 16 from 5,184 characters, four tiles per workgroup -- the
//       geometry that kernel's A/B runs settled on (72-line tiles, 243 of 256
//       lanes busy, four tiles per workgroup: profiles/r05/b64_geometry/) --
//       text double-buffered in LDS, each lane one block from one LDS window.
//       A text that is not flat (junk, '=' anywhere but "xx==" / "xxx=" in the
//       last group) is marked in redo[] and decoded again by the general
//       kernel, whose rule gives the same bytes on every flat text.
//
//   b64_update_flat_kernel   the piecewise pass of lbf_b64_update_launch,
//       between b64_update_lines_kernel and b64_update_kernel, one workgroup
//       per piece.  It takes the longest prefix of what the line kernel left
//       that it can show to be flat, a tile at a time: the carried group
//       completed from the next 4 - ncarry characters, then whole groups of
//       alphabet characters up to one that holds '='.  The prefix ends behind
//       a group, so nothing is carried.  Tiles are laid over the CHUNK (block u
//       of tile k holds chunk bytes [3888k + 16u, +16)), so a piece's first and
//       last tile are partial and a block that is not wholly the piece's is
//       written by bytes.  A tile is validated before it is stored; one with a
//       character outside the alphabet writes nothing and ends the prefix at
//       its start.  The kernel never finalises a chain.  tests/wire_flat_model.py
//       restates the rule and tests/test_b64_flat_cpu.py holds it to the
//       general one.
//
// A translation unit of its own: the other kernels' ISA stays as recorded.
// What it needs of kern_b64.hpp and b64_update_lines.hip (the staging, the
// table entry, the packing) is restated here.  DESIGN.md §4.7.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "b64_flat.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxCap = 1u << 30;        // the wire calls' bound on a chunk
constexpr uint64_t kMaxDecoded = 1ull << 61;  // b64_update_kernel's clamp
constexpr uint32_t kEq = 64, kSkip = 255;
constexpr uint32_t kTileBytes = 3888, kTileGroups = kTileBytes / 3, kTileText = 4 * kTileGroups;  // 1,296 / 5,184
constexpr uint32_t kTileBlocks = kTileBytes / 16;                                                 // 243
constexpr uint32_t kTilesPerGroup = 4;  // the one-shot pass: consecutive tiles of a chunk per workgroup
static_assert(kTileBytes % 48 == 0 && kTileBlocks <= kThreads, "whole groups, one 16-byte block per lane");
// A tile's text is staged as the aligned 16-byte blocks that hold it, behind
// kPad blocks: the first block of a piece reads its six-group window from up to
// 20 characters in front of the piece's first group (masked, but read).
constexpr uint32_t kPad = 2;
constexpr uint32_t kSpan = (kTileText + 15 + 15) / 16;  // 325 blocks: a tile at any phase
constexpr uint32_t kStage = kPad + kSpan + 2;           // and slack for the last window's 28-byte read
constexpr uint32_t kPer = (kSpan + kThreads - 1) / kThreads;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(lbf_b64_state) == 16 && offsetof(lbf_b64_state, decoded) == 0 &&
                  offsetof(lbf_b64_state, carry) == 8 && offsetof(lbf_b64_state, ncarry) == 12 &&
                  offsetof(lbf_b64_state, ended) == 13,
              "lbf_b64_state layout");

// The decode table entry of character c: 0..63, kEq for '=', kSkip otherwise.
__device__ __forceinline__ uint32_t value(uint32_t c) {
  return c - 'A' < 26u ? c - 'A' : c - 'a' < 26u ? c - 'a' + 26 : c - '0' < 10u ? c - '0' + 52 :
         c == '+' ? 62u : c == '/' ? 63u : c == '=' ? kEq : kSkip;
}

// Global bytes [src, src + len) into LDS as the aligned 16-byte blocks that
// hold them (a block that holds one byte of the span lies in its page): LDS
// byte 16 * kPad + (src mod 16) + k = src[k].  load() issues the loads, store()
// waits for them, so the tile in hand decodes while the next one's text flies.
struct Stage {
  u32x4 v[kPer];
  uint32_t blocks = 0;
  __device__ __forceinline__ void load(const uint8_t* src, uint32_t len) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const uint32_t phase = (uint32_t)(a & 15u);
    const u32x4* g = reinterpret_cast<const u32x4*>(a - phase);
    blocks = (phase + len + 15) / 16;  // at most kSpan
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (threadIdx.x + k * kThreads < blocks) v[k] = __builtin_nontemporal_load(g + threadIdx.x + k * kThreads);
  }
  __device__ __forceinline__ void store(uint4* lds) const {
    u32x4* l = reinterpret_cast<u32x4*>(lds) + kPad;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (threadIdx.x + k * kThreads < blocks) l[threadIdx.x + k * kThreads] = v[k];
  }
};

// The lane's six groups of a tile, g0 = 16 * lane / 3 onwards, from LDS bytes
// [c0, c0 + 24): one window of seven aligned dwords, each group cut out of it
// with v_alignbyte.  x[j] = group j's 24 bits, joined unmasked (a flagged
// group's bytes are never stored as data).  Table entries are 0..63, '=' 64 and
// anything else 255, so (entry >> 6) is 0 exactly for an alphabet character:
// two flag bits per group at 2j, for all four characters (*inner) and for the
// first two (*head).
__device__ __forceinline__ void six_groups(const uint8_t* sb, uint32_t c0, const uint8_t* tab, uint32_t x[6],
                                           uint32_t* inner, uint32_t* head) {
  const uint32_t* wb = reinterpret_cast<const uint32_t*>(sb) + (c0 >> 2);
  const uint32_t sh = c0 & 3u;  // the same in every lane: a group is four characters
  uint32_t win[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) win[k] = wb[k];
  uint32_t fi = 0, fh = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const uint32_t c = __builtin_amdgcn_alignbyte(win[j + 1], win[j], sh);
    const uint32_t s0 = tab[c & 255], s1 = tab[(c >> 8) & 255], s2 = tab[(c >> 16) & 255], s3 = tab[c >> 24];
    const uint32_t o2 = s0 | s1;
    fi |= ((o2 | s2 | s3) >> 6) << (2 * j);
    fh |= (o2 >> 6) << (2 * j);
    x[j] = (((s0 << 6) | s1) << 12) | ((s2 << 6) | s3);
  }
  *inner = fi;
  *head = fh;
}

// Bytes [phase, phase + 16) of the six groups' 18: group j's bytes are x[j]'s
// bytes 2, 1, 0, one v_perm_b32 per little-endian word (selector bytes 0-3
// pick from the second source, 4-7 from the first, 12 gives 0).
__device__ __forceinline__ uint4 pack16(const uint32_t x[6], uint32_t phase) {
  const uint32_t W0 = __builtin_amdgcn_perm(x[1], x[0], 0x06000102u);
  const uint32_t W1 = __builtin_amdgcn_perm(x[2], x[1], 0x05060001u);
  const uint32_t W2 = __builtin_amdgcn_perm(x[3], x[2], 0x04050600u);
  const uint32_t W3 = __builtin_amdgcn_perm(x[5], x[4], 0x06000102u);
  const uint32_t W4 = __builtin_amdgcn_perm(x[5], x[5], 0x0C0C0001u);
  return make_uint4(__builtin_amdgcn_alignbyte(W1, W0, phase), __builtin_amdgcn_alignbyte(W2, W1, phase),
                    __builtin_amdgcn_alignbyte(W3, W2, phase), __builtin_amdgcn_alignbyte(W4, W3, phase));
}

// The bytes of v at and past index `from` (0..16) zeroed.
__device__ __forceinline__ uint4 zero_from(uint4 v, uint32_t from) {
  uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t m = 0; m < 16; ++m)
    if (m >= from) ws[m >> 2] &= ~(255u << (8 * (m & 3)));
  return make_uint4(ws[0], ws[1], ws[2], ws[3]);
}

// Bytes [lo, hi) of the 16-byte block v to o[lo .. hi): one 16-byte store when
// that is all of it and o is aligned, bytes otherwise.  Nothing outside is written.
__device__ __forceinline__ void put_block(uint8_t* o, uint4 v, uint32_t lo, uint32_t hi) {
  if (lo == 0 && hi >= 16 && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
    *reinterpret_cast<uint4*>(o) = v;
    return;
  }
  const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t m = 0; m < 16; ++m)
    if (m >= lo && m < hi) o[m] = (uint8_t)(ws[m >> 2] >> (8 * (m & 3)));
}

// ---------------------------------------------------------------------------
// The one-shot pass.  blockIdx.x = group of tiles, blockIdx.y = chunk -
// chunk0.  Chunk i's text is text[text_off[i] .. + text_len[i]), text_len[i] =
// 4 * ceil(cap[i] / 3): G = text_len / 4 groups, the last of them "xxxx",
// "xxx=" or "xx==".  Tile k reads characters [5184k, +5184) and writes bytes
// [3888k, +3888), so the text's tiles cover the slot.  out[out_off[i] .. +
// cap[i]): the decoded bytes, zeros behind a short decode, nothing at or past
// cap.  sizes[i] = min(decoded, cap[i]), over[i] = decoded > cap[i] (the
// one-pass decode's contract, kern_b64.hpp).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) b64_flat_decode_kernel(B64FlatDecode b) {
  __shared__ uint4 stage[2][kStage];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t last_shared;
  const uint32_t i = b.chunk0 + blockIdx.y, t0 = blockIdx.x * kTilesPerGroup;
  const uint32_t len = b.text_len[i], limit = b.cap[i];
  // the host routes candidates only; any other length is the general decode's (the whole workgroup leaves)
  if (len == 0 || limit > kMaxCap || (uint64_t)len != 4 * (((uint64_t)limit + 2) / 3)) {
    if (t0 == 0 && threadIdx.x == 0) b.redo[i] = 1;
    return;
  }
  const uint32_t groups = len / 4;
  const uint32_t own = (len + kTileText - 1) / kTileText;
  if (t0 >= own) return;  // the whole workgroup: no barrier below is reached
  const uint32_t t1 = min(own, t0 + kTilesPerGroup);
  const uint8_t* const t = b.text + b.text_off[i];
  uint8_t* const o = b.out + b.out_off[i];
  const uint32_t delta = 16 * kPad + (uint32_t)(reinterpret_cast<uintptr_t>(t) & 15u);  // of every tile: 5,184 = 16 * 324
  Stage st;
  auto load = [&](uint32_t tile) {
    const uint32_t tbeg = tile * kTileText;  // below len
    st.load(t + tbeg, min(kTileText, len - tbeg));
  };
  load(t0);
  tab[threadIdx.x] = (uint8_t)value(threadIdx.x);
  if (threadIdx.x == 0) {
    // the last group -- "xxxx", "xxx=" or "xx==" -- sets the decoded length
    const uint32_t at = 4 * (groups - 1);
    const uint32_t c2 = value(t[at + 2]), c3 = value(t[at + 3]);
    const uint32_t last = c3 < 64 ? 3u : c2 < 64 ? 2u : 1u;
    last_shared = last;
    if (t0 == 0) {
      const uint64_t want = 3ull * (groups - 1) + last;
      b.sizes[i] = (uint32_t)min<uint64_t>(want, limit);
      b.over[i] = want > limit ? 1 : 0;
      if (c3 == kSkip || c2 == kSkip || (c2 == kEq && c3 != kEq)) b.redo[i] = 1;
    }
  }
  st.store(stage[0]);
  __syncthreads();
  const uint32_t want = 3 * (groups - 1) + last_shared;  // at most 2^30 + 2
  bool bad = false;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    const uint32_t buf = (tile - t0) & 1u;
    if (tile + 1 < t1) load(tile + 1);  // in flight while this tile decodes
    const uint32_t b0 = 16 * threadIdx.x, pos = tile * kTileBytes + b0;
    if (threadIdx.x < kTileBlocks && pos < limit) {
      const uint32_t g0 = b0 / 3, phase = b0 - 3 * g0;
      uint32_t x[6], inner, head;
      six_groups(reinterpret_cast<const uint8_t*>(stage[buf]), delta + 4 * g0, tab, x, &inner, &head);
      // window groups j < rel lie in front of the chunk's last group (all four characters of the alphabet);
      // group rel is the last (its first two of the alphabet; lane 0 checked its padding); those behind
      // it were decoded from whatever lay in LDS, and their bytes lie at or past `want`
      const int32_t rel = (int32_t)groups - 1 - (int32_t)(tile * kTileGroups + g0);  // >= 0: pos < limit <= 3 * groups
      const uint32_t nin = (uint32_t)min(rel, 6);
      const uint32_t head_mask = rel < 6 ? 3u << (2 * rel) : 0u;
      bad |= ((inner & ((1u << (2 * nin)) - 1u)) | (head & head_mask)) != 0;
      uint4 v = pack16(x, phase);
      if (pos + 16 > want) v = zero_from(v, want > pos ? want - pos : 0u);  // zeros behind a short decode
      put_block(o + pos, v, 0u, limit - pos);
    }
    if (tile + 1 < t1) {
      st.store(stage[buf ^ 1u]);  // that buffer's last reader was the previous tile, before the last barrier
      __syncthreads();
    }
  }
  if (bad) b.redo[i] = 1;  // every writer stores the same 1
}

// ---------------------------------------------------------------------------
// The piecewise pass.  blockIdx.x = piece.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) b64_update_flat_kernel(B64FlatParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written, the hand-off included
  __shared__ uint4 stage[2][kStage];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t wave_bad[2][kThreads / 64];

  uint8_t* const rec = p.b64_states + 16 * si;
  const uint4 r = *reinterpret_cast<const uint4*>(rec);
  uint64_t decoded = (uint64_t)r.x | ((uint64_t)r.y << 32);
  if (decoded > kMaxDecoded) decoded = kMaxDecoded;  // b64_update_kernel's clamps, all three
  const uint32_t nc = r.w & 3u;
  const uint32_t carry = r.z & ((1u << (6u * nc)) - 1u);
  const bool ended = ((r.w >> 8) & 0xFFu) != 0;
  const uint32_t cap = p.cap[i], piece_len = p.text_len[i];
  uint32_t skip = 0;  // the characters the line kernel took
  if (p.after_lines) {
    skip = p.taken[i];
    if (skip > piece_len) skip = piece_len;  // never: the line path takes a prefix
  }
  const uint32_t len = piece_len - skip;
  // a record the batch call would refuse, or nothing to take: the rest is b64_update_kernel's whole
  if (cap > kMaxCap || ended || decoded % 3 != 0 || len == 0) {
    if (threadIdx.x == 0) {
      if (!p.after_lines) {
        p.before[i] = decoded;
        p.taken[i] = 0;
      }
      if (p.flat_chars) p.flat_chars[i] = 0;
    }
    return;  // the whole workgroup: every value above is the same in every lane
  }
  const uint8_t* const t = p.text + p.text_off[i] + skip;
  const uint64_t slot = p.out_off[i];  // positions are sums of 64-bit numbers, taken mod 2^64
  tab[threadIdx.x] = (uint8_t)value(threadIdx.x);

  // ---- the head: the carried group.  Every lane works it out; lane 0 writes.
  uint64_t D = decoded;  // bytes of the chain decoded so far; a multiple of 3 from here on
  uint32_t pos = 0;      // characters of the remainder taken so far
  bool go = true;
  if (nc != 0) {
    const uint32_t need = 4 - nc;
    uint32_t x = 0, junk = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k)
      if (k < nc) x |= ((carry >> (6u * k)) & 63u) << (18u - 6u * k);
    if (len < need) {
      go = false;
    } else {
#pragma unroll
      for (uint32_t k = 1; k < 4; ++k) {
        if (k < nc) continue;
        const uint32_t v = value(t[k - nc]);
        junk |= v >> 6;
        x |= (v & 63u) << (18u - 6u * k);
      }
      go = junk == 0;
    }
    if (go) {
      if (threadIdx.x == 0) {
        uint8_t* const o = p.out + (slot + D);
        if (D < cap) o[0] = (uint8_t)(x >> 16);
        if (D + 1 < cap) o[1] = (uint8_t)(x >> 8);
        if (D + 2 < cap) o[2] = (uint8_t)x;
      }
      D += 3;  // at most 2^61 + 1: no wrap
      pos = need;
    }
  }
  uint32_t groups = 0;  // whole groups that follow, by the remainder's length
  if (go) {
    groups = (len - pos) / 4;
    if (groups) {  // '=' stops the prefix: only the last group of a text holds it
      const uint8_t* const g = t + pos + 4 * (groups - 1);
      if (g[0] == '=' || g[1] == '=' || g[2] == '=' || g[3] == '=') --groups;
    }
  }

  // ---- the tiles of the chunk that hold groups [D / 3, D / 3 + groups)
  uint32_t done = 0;  // groups of validated tiles
  if (groups) {
    const uint64_t tile0 = D / kTileBytes;
    const uint32_t g_first = (uint32_t)(D - tile0 * kTileBytes) / 3;  // the first group's index in its tile
    const uint32_t g_end = g_first + groups;                          // < 2^30 + 1,296
    const uint32_t ntiles = (g_end + kTileGroups - 1) / kTileGroups;
    Stage st;
    uint32_t delta_next = 0;
    // tile j's groups [gl, gh) of the tile; character c of the tile is character pos + (5184 j + c) - 4 g_first
    // of the remainder
    auto load = [&](uint32_t j) {
      const uint32_t gl = j == 0 ? g_first : 0u;
      const uint32_t gh = g_end - j * kTileGroups < kTileGroups ? g_end - j * kTileGroups : kTileGroups;
      const uint8_t* const src = t + pos + ((uint64_t)j * kTileText + 4 * gl - 4 * g_first);
      st.load(src, 4 * (gh - gl));
      delta_next = 16 * kPad + (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u) - 4 * gl;  // mod 2^32
    };
    load(0);
    st.store(stage[0]);
    uint32_t delta = delta_next;
    __syncthreads();  // the table and tile 0's text
    for (uint32_t j = 0; j < ntiles; ++j) {
      const uint32_t buf = j & 1u;
      const bool next = j + 1 < ntiles;
      if (next) load(j + 1);  // in flight while this tile decodes
      const uint32_t gl = j == 0 ? g_first : 0u;
      const uint32_t gh = g_end - j * kTileGroups < kTileGroups ? g_end - j * kTileGroups : kTileGroups;
      const uint32_t b0 = 16 * threadIdx.x;
      // the lanes whose block holds a byte of groups [gl, gh)
      const bool mine = threadIdx.x < kTileBlocks && b0 + 16 > 3 * gl && b0 < 3 * gh;
      bool bad = false;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (mine) {
        // g0 >= gl - 5 and g0 < gh: the window starts at most 20 characters in front of the staged text (the pad)
        const uint32_t g0 = b0 / 3, phase = b0 - 3 * g0;
        uint32_t x[6], inner, head;
        six_groups(reinterpret_cast<const uint8_t*>(stage[buf]), delta + 4 * g0, tab, x, &inner, &head);
        const uint32_t jl = gl > g0 ? gl - g0 : 0u, jh = gh - g0 < 6u ? gh - g0 : 6u;
        bad = (inner & ((1u << (2 * jh)) - 1u) & ~((1u << (2 * jl)) - 1u)) != 0;  // the piece's groups only
        v = pack16(x, phase);
      }
      const bool wave_has = __ballot(bad) != 0;
      if ((threadIdx.x & 63u) == 0) wave_bad[buf][threadIdx.x >> 6] = wave_has ? 1u : 0u;
      if (next) {
        st.store(stage[buf ^ 1u]);  // that buffer's last readers were the previous tile's lanes, before its barrier
        delta = delta_next;
      }
      __syncthreads();  // the flags of this tile, the text of the next
      // (wave_bad[buf] is written again two tiles on, behind the next tile's barrier)
      if (wave_bad[buf][0] | wave_bad[buf][1] | wave_bad[buf][2] | wave_bad[buf][3]) break;  // the whole workgroup
      done += gh - gl;
      if (!mine) continue;
      // the tile is good: the block's bytes that are the piece's and lie below cap
      const uint64_t tb = (tile0 + j) * kTileBytes;  // at most 2^61 + 3,888
      const uint32_t in_cap = cap > tb ? (cap - tb < kTileBytes ? (uint32_t)(cap - tb) : kTileBytes) : 0u;
      const uint32_t wlo = 3 * gl, whi = 3 * gh < in_cap ? 3 * gh : in_cap;
      if (whi > b0)
        put_block(p.out + (slot + tb + b0), v, wlo > b0 ? wlo - b0 : 0u, whi - b0);
    }
  }
  if (threadIdx.x != 0) return;
  const uint32_t took = go ? pos + 4 * done : 0u;
  const uint64_t now = D + 3ull * done;
  if (go && now != decoded)  // the prefix ends behind a group: nothing is carried
    *reinterpret_cast<uint4*>(rec) = make_uint4((uint32_t)(now < kMaxDecoded ? now : kMaxDecoded),
                                                (uint32_t)((now < kMaxDecoded ? now : kMaxDecoded) >> 32), 0u, 0u);
  if (!p.after_lines) p.before[i] = decoded;
  p.taken[i] = skip + took;
  if (p.flat_chars) p.flat_chars[i] = took;
}

}  // namespace

// grid = (groups of kTilesPerGroup tiles, chunks), in launches of at most 65,535 chunks (grid.y)
int launch_b64_flat_decode(const B64FlatDecode& b, hipStream_t stream) {
  if (b.n == 0) return LBF_OK;
  const uint32_t tiles = std::max(1u, (b.max_text_len + kTileText - 1) / kTileText);
  constexpr uint32_t kPerLaunch = 65535;
  for (uint32_t c0 = 0; c0 < b.n; c0 += kPerLaunch) {
    B64FlatDecode s = b;
    s.chunk0 = b.chunk0 + c0;
    s.n = std::min(kPerLaunch, b.n - c0);
    hipLaunchKernelGGL(b64_flat_decode_kernel, dim3((tiles + kTilesPerGroup - 1) / kTilesPerGroup, s.n), dim3(kThreads),
                       0, stream, s);
    LBF_HIP_TRY(hipGetLastError());
  }
  return LBF_OK;
}

int launch_b64_update_flat(const B64FlatParams& p, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(b64_update_flat_kernel, dim3(n), dim3(kThreads), 0, stream, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace lbf

// The flat path's switch: LBF_B64_FLAT at first use, then lbf_set_b64_flat.
static std::atomic<int> g_b64_flat{-1};

bool lbf::b64_flat_enabled() {
  int v = g_b64_flat.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("LBF_B64_FLAT");
    const int from_env = lbf::kB64FlatDefault ? !(e && e[0] == '0' && e[1] == 0) : (e && e[0] == '1' && e[1] == 0);
    g_b64_flat.compare_exchange_strong(v, from_env, std::memory_order_relaxed);  // a setter that got in first wins
    v = g_b64_flat.load(std::memory_order_relaxed);
  }
  return v != 0;
}

extern "C" int lbf_set_b64_flat(int on) {
  const int before = lbf::b64_flat_enabled() ? 1 : 0;
  g_b64_flat.store(on ? 1 : 0, std::memory_order_relaxed);
  return before;
}
