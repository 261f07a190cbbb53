// b64_decode_tiles.hpp -- the tiles of the one-shot base64 decode as device
// functions: the geometry of a tile of whole lines, its staging, the
// encoder-layout (canon) pass's length rule, block and tile, and the two tile
// bodies -- what one workgroup does with its group of tiles of one chunk --
// b64_canon_decode_tiles and b64_flat_decode_tiles.  b64_decode_routed_kernel
// (b64_verify_launch.hip) calls whichever body a chunk's own lengths ask for,
// so text of both layouts shares one launch in caller order.
//
// Every function is __device__ __forceinline__ and the header defines no kernel,
// no __constant__ and no __shared__ (the callers own the LDS and pass it in):
// including it adds no symbol to a translation unit.  The staging, the length
// rule, the block, the tile and zero_from are stated here once (the geometry's
// constants here and, for the units that hold its kernels, in kern_b64.hpp), and
// b64_decode_canon_kernel (kern_b64.hpp, in sha1_kernels.hip) and
// b64_flat_decode_kernel (b64_flat.hip) are built from them.  The two BODIES
// are those kernels' bodies written out again: called from the old kernels,
// every form tried (the whole body; the body behind the length check; tables by
// reference, by value, with and without __restrict__) changed the instruction
// streams tests/golden/isa_shipped.json and tests/golden/isa_b64.json pin --
// the callee is simplified on its own before it is inlined, and the scheduler
// then orders the same instructions differently -- so the old kernels keep
// their text.  A change to a body here belongs in its kernel too; DESIGN.md
// §4.5 says so, and tests/test_gpu_b64_verify_launch.py holds the routed kernel
// to lbf_b64_verify_batch, which runs the old ones.
//
// Each body is taken by the whole workgroup: what it branches on in front of a
// barrier (the chunk's lengths, the workgroup's place in the grid) is the same
// in every lane.  DESIGN.md §4.5.
#pragma once

#include <hip/hip_runtime.h>

#include "b64_device.hpp"
#include "b64_encode_update.hpp"
#include "b64_flat.hpp"
#include "b64_update_stages.hpp"
#include "lbf_internal.hpp"

// The geometry of the tiles of whole lines, as kern_b64.hpp states it (with the
// runs that settled it): that header holds kernels, so a unit that must not
// compile them a second time gets the same constants from here.
#ifndef LBF_B64_TILE_GEOMETRY_STATED
namespace lbf {
namespace {

using b64d::kEq;
using b64d::kSkip;
constexpr int kB64Threads = 256;  // one lane per entry of the decode table

// The encode's tile: 112 lines, 6,048 bytes -> 8,176 characters.
#ifndef LBF_B64_ENC_LINES
#define LBF_B64_ENC_LINES 112
#endif
constexpr uint32_t kB64TileLines = LBF_B64_ENC_LINES;
constexpr uint32_t kB64TileText = kB64TileLines * 73;    // 8,176 characters
constexpr uint32_t kB64TileBytes = kB64TileLines * 54;   // 6,048 bytes
constexpr uint32_t kB64TileGroups = kB64TileLines * 18;  // 2,016 groups
// The decode's tile: 72 lines, 5,256 characters -> 3,888 bytes, 243 of the 256 lanes busy.
#ifndef LBF_B64_DEC_LINES
#define LBF_B64_DEC_LINES 72
#endif
#ifndef LBF_B64_DEC_WIN64
#define LBF_B64_DEC_WIN64 0
#endif
constexpr uint32_t kDecLines = LBF_B64_DEC_LINES;
constexpr uint32_t kDecText = kDecLines * 73, kDecBytes = kDecLines * 54, kDecGroups = kDecLines * 18;
// Consecutive tiles of a chunk per workgroup, double-buffered in LDS.
#ifndef LBF_B64_DEC_TILES_PER_GROUP
#define LBF_B64_DEC_TILES_PER_GROUP 4
#endif
#ifndef LBF_B64_ENC_TILES_PER_GROUP
#define LBF_B64_ENC_TILES_PER_GROUP 2
#endif
constexpr uint32_t kDecTilesPerGroup = LBF_B64_DEC_TILES_PER_GROUP, kEncTilesPerGroup = LBF_B64_ENC_TILES_PER_GROUP;

}  // namespace
}  // namespace lbf
#endif  // LBF_B64_TILE_GEOMETRY_STATED

namespace lbf {
namespace {

// whichever header stated the geometry, it is this one
static_assert(kB64Threads == 256 && kB64TileText == kB64TileLines * 73 && kB64TileBytes == kB64TileLines * 54 &&
                  kDecText == kDecLines * 73 && kDecBytes == kDecLines * 54 && kDecGroups == kDecLines * 18,
              "a line is 73 characters, 54 bytes, 18 groups");
static_assert(kB64TileText % 16 == 0 && kB64TileBytes % 16 == 0 && kDecBytes % 16 == 0, "tiles of 16-byte blocks");
#if LBF_B64_DEC_LINES == 72 && LBF_B64_DEC_TILES_PER_GROUP == 4  // the geometry of record (A/B builds set others)
static_assert(kDecText == b64s::kLineTileText && kDecBytes == b64s::kTileBytes, "the piecewise decode's tile of lines");
#endif

// A tile's span staged through registers into LDS (b64_device.hpp): LDS byte (delta + k) = src[k].
template <uint32_t kPer>
using B64Stage = b64d::Stage<kPer, kB64Threads, 0>;

// Store a 16-byte block to base + pos, clipped to [0, end) of the slot: 64-bit
// positions, and the byte tail as the loop that stops at the slot's end.
__device__ __forceinline__ void b64_put_block(uint8_t* base, uint64_t pos, uint64_t end, uint4 v) {
  b64d::put_block<true, true>(base, pos, (uint64_t)0, end, v);
}

// ---------------------------------------------------------------------------
// One pass for text laid out as the encoder writes it (round 4; tiled in
// round 5).  Almost every frame carries exactly what xmlrpc++'s encoder
// wrote: group g of the chunk at 4g + g/18, a separator (any character outside
// the alphabet) after every 18th group, '=' only as "xx==" / "xxx=" in the
// last group.  For such a text the place of every character is known without
// a scan.  The lanes check the layout as they read it; a chunk whose text
// breaks it anywhere (junk, a dropped or extra character, '=' elsewhere) is
// marked in redo[] and decoded again by the general rule (b64_decode_kernel,
// or b64_decode_scan_kernel behind the routed kernel), which gives the same
// result as this pass on every canonical text.
//
// The length gives the group count.  The encoder writes a separator after
// every 18th complete group, so a text of G = 18q + r groups (0 < r < 18 or
// r = 0) has length 73q + 4r, and one whose last, padded group is the 18th of
// its line has no separator after it: 73q + 72, G = 18(q + 1).
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool b64_canon_groups(uint32_t len, uint32_t* groups) {
  const uint32_t q = len / 73, rem = len % 73;
  if (rem == 72) {  // the last line's 18th group is the padded last group
    *groups = 18 * q + 18;
    return true;
  }
  if (rem % 4 != 0) return false;
  *groups = 18 * q + rem / 4;
  return true;
}

// One block of a tile of the one-pass decode from its text in LDS (sb, from
// byte `delta`): in pass p, lane v builds and stores bytes [16u, 16u + 16) of
// the tile, u = v + 256p (if the tile has that block).  Returns true when the
// lane saw a character that breaks the layout.  The kernel is VALU-bound
// (about 70 % of its time was VALU issue at 230 instructions per block), so the
// block keeps its instruction count down: the layout checks fold into two flag
// words, the sextets are joined unmasked, and the 18 bytes are packed with five
// v_perm_b32 (157 -> 133 us per 1,024 x 256 KiB).
template <uint32_t kPass>
__device__ __forceinline__ bool b64_decode_block(const uint8_t* sb, uint32_t delta, const uint8_t* tab, uint32_t tile,
                                                 uint32_t groups, uint32_t len, uint64_t want, uint32_t limit,
                                                 uint8_t* o) {
  if (threadIdx.x + kPass * kB64Threads >= kDecBytes / 16) return false;
  // Bytes [16u, 16u + 16) of the tile come from its groups g0 .. g0 + 5, whose
  // characters lie in [c0, c0 + 25): 24 characters and at most one separator,
  // after group 17 - r0 of the window when r0 >= 12.  One window of eight
  // aligned dwords holds them; each group's four characters are cut out of it
  // with v_alignbyte (no divergent branch: groups past the chunk's end are
  // decoded from whatever lies there and masked below).
  const uint32_t* w = reinterpret_cast<const uint32_t*>(sb);
  const uint32_t b0 = 16 * (threadIdx.x + kPass * kB64Threads), g0 = b0 / 3, phase = b0 - 3 * g0;
  const uint32_t l0 = g0 / 18, r0 = g0 - 18 * l0;
  const uint32_t c0 = delta + 4 * g0 + l0, sh0 = c0 & 3u;
#if LBF_B64_DEC_WIN64
  // A/B: the window as five 8-byte reads from the even dword below it.  Lanes'
  // windows start ~5.3 dwords apart, so eight ds_read_b32 (banks (a/4) mod 32,
  // 32-lane groups) meet ~3-way bank conflicts; ds_read_b64 banks mod 64.
  const uint32_t r = (c0 >> 2) & 1u;
  const uint2* wb = reinterpret_cast<const uint2*>(w + ((c0 >> 2) & ~1u));
  uint32_t win[10];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const uint2 x2 = wb[k];
    win[2 * k] = x2.x;
    win[2 * k + 1] = x2.y;
  }
#else
  const uint32_t* wb = w + (c0 >> 2);
  uint32_t win[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) win[k] = wb[k];
#endif
  const uint32_t gbase = tile * kDecGroups + g0;  // the chunk's index of group g0
  bool bad = false;
  uint32_t x[6];
  // Table entries are 0..63, '=' 64 and anything else 255, so (entry >> 6)
  // is 0 exactly for an alphabet character: two flag bits per group, at 2j,
  // for all four characters (finner) and the first two (fhead).
  uint32_t finner = 0, fhead = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const uint32_t sep = r0 + j >= 18 ? 1u : 0u;
    const uint32_t off = sh0 + sep;  // 0..4: this group's offset from dword j of the window
#if LBF_B64_DEC_WIN64
    const uint32_t q = r + (off >> 2);  // 0..2 dwords past win[j]
    const uint32_t lo = q == 0 ? win[j] : q == 1 ? win[j + 1] : win[j + 2];
    const uint32_t hi = q == 0 ? win[j + 1] : q == 1 ? win[j + 2] : win[j + 3];
#else
    const uint32_t lo = off >= 4 ? win[j + 1] : win[j], hi = off >= 4 ? win[j + 2] : win[j + 1];
#endif
    const uint32_t c = __builtin_amdgcn_alignbyte(hi, lo, off & 3u);
    const uint32_t s0 = tab[c & 255], s1 = tab[(c >> 8) & 255], s2 = tab[(c >> 16) & 255], s3 = tab[c >> 24];
    const uint32_t o2 = s0 | s1, o4 = o2 | s2 | s3;
    finner |= (o4 >> 6) << (2 * j);
    fhead |= (o2 >> 6) << (2 * j);
    // unmasked: an entry above 63 spoils only its own group's bytes, and such a
    // group is either marked bad or the last group's '=' padding, whose bytes
    // (those a '=' in character 2 or 3 reaches) lie past the decoded length
    // and are zeroed below
    x[j] = (((s0 << 6) | s1) << 12) | ((s2 << 6) | s3);
  }
  {
    // window groups j < rel lie inside the text (all four characters in the
    // alphabet); group rel is the chunk's last (its first two in the alphabet;
    // the kernel checks its padding)
    const int32_t rel = (int32_t)groups - 1 - (int32_t)gbase;
    const uint32_t nin = (uint32_t)min(max(rel, 0), 6);
    const uint32_t inner_mask = (1u << (2 * nin)) - 1u;
    const uint32_t head_mask = rel >= 0 && rel < 6 ? 3u << (2 * rel) : 0u;
    bad |= ((finner & inner_mask) | (fhead & head_mask)) != 0;
  }
  // the separator after group 17 - r0 (when in the window): any character outside the alphabet
  {
    const uint32_t js = 17 - r0;  // < 6 when r0 >= 12
    const uint32_t gs = gbase + js;
    const uint32_t at = (c0 & ~3u) + min(sh0 + 4 * js + 4, 31u);
    const bool check = r0 >= 12 && 4 * gs + gs / 18 + 4 < len;
    bad |= check && tab[sb[at]] != kSkip;
  }
  uint4 v = b64d::pack16(x, phase);  // the 18 bytes of the six groups, cut to the block's 16
  const uint64_t pos = (uint64_t)tile * kDecBytes + b0;
  if (pos < limit) {
    if (pos + 16 > want) {  // the decoded bytes end inside this block: zero the rest of the slot
      uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int m = 0; m < 16; ++m)
        if (pos + m >= want) ws[m >> 2] &= ~(255u << (8 * (m & 3)));
      v = make_uint4(ws[0], ws[1], ws[2], ws[3]);
    }
    b64_put_block(o, pos, limit, v);
  }
  return bad;
}

// A tile: every lane its block of each pass (one pass for the shipped 243-block
// tile; the block index is written out in each pass rather than passed in, which
// kept the shipped kernel at 71 VGPRs where a block-index argument made it 87).
__device__ __forceinline__ bool b64_decode_tile(const uint8_t* sb, uint32_t delta, const uint8_t* tab, uint32_t tile,
                                                uint32_t groups, uint32_t len, uint64_t want, uint32_t limit,
                                                uint8_t* o) {
  static_assert(kDecBytes / 16 <= 3 * kB64Threads, "three blocks per lane at most");
  bool bad = b64_decode_block<0>(sb, delta, tab, tile, groups, len, want, limit, o);
  if constexpr (kDecBytes / 16 > kB64Threads) bad |= b64_decode_block<1>(sb, delta, tab, tile, groups, len, want, limit, o);
  if constexpr (kDecBytes / 16 > 2 * kB64Threads)
    bad |= b64_decode_block<2>(sb, delta, tab, tile, groups, len, want, limit, o);
  return bad;
}

// The canon body's stage buffer, in 16-byte blocks: a tile's span, its phase,
// and slack for the last lane's 32-byte window read
constexpr uint32_t kCanonStage = (kDecText + 15 + 15) / 16 + 2;

// The encoder-layout body, for the workgroup that has tiles [t0, t0 +
// kDecTilesPerGroup) of chunk i.  Chunk i's text is text[text_off[i] .. +
// text_len[i]); its decoded bytes go to out[out_off[i] .. + cap[i]): bytes
// [0, min(decoded, cap)) decoded, the rest of the slot zeroed, so a short text
// never leaves stale device bytes in the caller's slot.  sizes[i] =
// min(decoded, cap[i]), over[i] = decoded > cap[i].  A text whose length is not
// an encoder's, or that breaks the layout anywhere, is marked in redo[i].
// `stage`, `tab` and `last_shared` are the workgroup's LDS.
__device__ __forceinline__ void b64_canon_decode_tiles(const uint8_t* __restrict__ text,
                                                       const uint64_t* __restrict__ text_off,
                                                       const uint32_t* __restrict__ text_len,
                                                       uint8_t* __restrict__ out,
                                                       const uint64_t* __restrict__ out_off,
                                                       const uint32_t* __restrict__ cap, uint32_t* __restrict__ sizes,
                                                       uint8_t* __restrict__ over, uint8_t* __restrict__ redo,
                                                       uint32_t i, uint32_t t0, uint4 (*stage)[kCanonStage],
                                                       uint8_t* tab, uint32_t& last_shared) {
  constexpr uint32_t kPer = (kCanonStage + kB64Threads - 1) / kB64Threads;  // staged blocks per lane
  const uint32_t len = text_len[i];
  uint32_t groups = 0;
  if (!b64_canon_groups(len, &groups)) {  // the whole workgroup leaves: no barrier below is reached
    if (t0 == 0 && threadIdx.x == 0) redo[i] = 1;
    return;
  }
  const uint32_t limit = cap[i];
  // the tiles this chunk has: its text's and its slot's (at least one, for the sizes)
  const uint32_t own = max(1u, max((len + kDecText - 1) / kDecText,
                                   (limit + kDecBytes - 1) / kDecBytes));
  if (t0 >= own) return;  // the whole workgroup
  const uint32_t t1 = min(own, t0 + kDecTilesPerGroup);
  const uint8_t* t = text + text_off[i];
  uint8_t* o = out + out_off[i];
  B64Stage<kPer> st;
  auto load = [&](uint32_t tile) {
    const uint32_t tbeg = tile * kDecText;
    st.clear();
    if (tbeg < len) st.load(t + tbeg, min(kDecText, len - tbeg));
  };
  load(t0);
  tab[threadIdx.x] = (uint8_t)b64d::value(threadIdx.x);
  if (threadIdx.x == 0) {
    // the last group -- "xxxx", "xxx=" or "xx==" -- sets the decoded length
    uint32_t last = 3;
    bool bad = false;
    if (groups > 0) {
      const uint32_t g = groups - 1, at = 4 * g + g / 18;
      const uint32_t c2 = b64d::value(t[at + 2]), c3 = b64d::value(t[at + 3]);
      last = c3 < 64 ? 3u : c2 < 64 ? 2u : 1u;
      bad = c3 == kSkip || c2 == kSkip || (c2 == kEq && c3 != kEq);
    }
    last_shared = last;
    if (t0 == 0) {
      const uint64_t want = groups ? 3ull * (groups - 1) + last : 0;
      sizes[i] = (uint32_t)min<uint64_t>(want, limit);
      over[i] = want > limit ? 1 : 0;
      if (bad) redo[i] = 1;
    }
  }
  st.store(stage[0]);
  uint32_t delta = st.delta;
  __syncthreads();
  const uint64_t want = groups ? 3ull * (groups - 1) + last_shared : 0;
  bool bad = false;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    const uint32_t buf = (tile - t0) & 1u;
    if (tile + 1 < t1) load(tile + 1);  // in flight while this tile decodes
    bad |= b64_decode_tile(reinterpret_cast<const uint8_t*>(stage[buf]), delta, tab, tile, groups, len, want, limit, o);
    if (tile + 1 < t1) {
      st.store(stage[buf ^ 1u]);  // that buffer's last reader was the previous tile, before the last barrier
      delta = st.delta;
      __syncthreads();
    }
  }
  if (bad) redo[i] = 1;  // every writer stores the same 1
}

}  // namespace
}  // namespace lbf

namespace lbf {
namespace b64s {

// The tile of the flat body is b64_update_stages.hpp's: kTileBytes = 3888 bytes
// (243 blocks of 16, 1,296 groups) from kFlatTileText = 5184 characters.
constexpr uint32_t kFlatTilesPerGroup = 4;  // the one-shot pass: consecutive tiles of a chunk per workgroup

// The bytes of v at and past index `from` (0..16) zeroed.
__device__ __forceinline__ uint4 zero_from(uint4 v, uint32_t from) {
  uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (uint32_t m = 0; m < 16; ++m)
    if (m >= from) ws[m >> 2] &= ~(255u << (8 * (m & 3)));
  return make_uint4(ws[0], ws[1], ws[2], ws[3]);
}

// The flat body, for the workgroup that has tiles [t0, t0 + kFlatTilesPerGroup)
// of chunk i, a candidate of the flat pass (b64_flat.hpp): len = text_len[i] =
// 4 * ceil(limit / 3) > 0 with limit = cap[i] at most kMaxCap, so G = len / 4
// groups, the last of them "xxxx", "xxx=" or "xx==".  Tile k reads characters
// [5184k, +5184) and writes bytes [3888k, +3888), so the text's tiles cover the
// slot.  out[out_off[i] .. + cap[i]): the decoded bytes, zeros behind a short
// decode, nothing at or past cap.  sizes[i] = min(decoded, cap[i]), over[i] =
// decoded > cap[i] (the one-pass decode's contract).  A text that is not flat
// is marked in redo[i].  `stage`, `tab` and `last_shared` are the workgroup's LDS.
__device__ __forceinline__ void b64_flat_decode_tiles(const B64FlatDecode& b, uint32_t i, uint32_t t0, uint32_t len,
                                                      uint32_t limit, uint4 (*stage)[kStage], uint8_t* tab,
                                                      uint32_t& last_shared) {
  constexpr uint32_t kTileText = kFlatTileText, kTilesPerGroup = kFlatTilesPerGroup;
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

}  // namespace b64s
}  // namespace lbf
