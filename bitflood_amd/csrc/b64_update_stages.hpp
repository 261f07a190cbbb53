// b64_update_stages.hpp -- the three stages of the piecewise base64 decode as
// device functions: the line stage (tiles of whole lines of xmlrpc++'s layout),
// the flat stage (tiles of unbroken text) and the general scan.  Each works on
// one piece with one workgroup of 256 lanes, on a chain record held in
// registers and on LDS the caller owns, and takes a prefix of the text it is
// given; what it took moves the record on.
//
// Two kinds of kernel are built from them.  b64_update_lines_kernel,
// b64_update_flat_kernel and b64_update_kernel (b64_update_lines.hip,
// b64_flat.hip, b64_update.hip) run one stage each and hand the record on
// through global memory and two numbers through the piece table's arrays;
// b64_update_fused_kernel (b64_update_fused.hip) runs all three in one launch
// and keeps the record in registers.  The rules are stated where they were
// first written: b64_update_lines.hip, b64_flat.hip, b64_update.hip.
//
// Every branch that holds a barrier is taken by the whole workgroup: the
// record, the piece's length and what a stage took are the same in every lane,
// and no function here leaves early in some lanes only.  DESIGN.md §4.7.
//
// The staging, the table entry, the block store, the packing, the window of
// unbroken text and the scan's prefix sum are b64_device.hpp's, shared with the
// one-shot kernels.  The window of a tile of lines (decode_line_block) is
// kern_b64.hpp's b64_decode_block written out again: as a shared function it
// changes the recorded ISA of b64_update_seq_kernel and of the one-pass decode.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "b64_device.hpp"
#include "b64_encode_update.hpp"
#include "lbf_hash.h"

namespace lbf {
namespace b64s {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kMaxCap = (uint32_t)b64e::kEncMaxChunk;  // the wire calls' bound on a chunk
// A chain's byte count stays at or below this (the host call refuses a record at
// or past it).  read_rec clamps what it loads to it and a piece adds less than
// 2^32, so no position ever wraps, whatever a forged record claims.
constexpr uint64_t kMaxDecoded = 1ull << 61;
// Tiles are laid over the CHUNK: block u of tile k holds chunk bytes [3888k +
// 16u, +16), from 72 lines (5,256 characters) or 5,184 unbroken characters.
constexpr uint32_t kTileBytes = 3888, kTileGroups = kTileBytes / 3, kTileBlocks = kTileBytes / 16;  // 1,296 / 243
constexpr uint32_t kLineTileText = 72 * 73, kFlatTileText = 4 * kTileGroups;
static_assert(kTileBytes % 48 == 0 && kTileBlocks <= kThreads, "whole groups, one 16-byte block per lane");
// A tile's text is staged as the aligned 16-byte blocks that hold it, behind
// kPad blocks: the first block of a piece reads its six-group window from up to
// 24 characters in front of the piece's first group (masked, but read).
constexpr uint32_t kPad = 2;
constexpr uint32_t kSpan = (kLineTileText + 15 + 15) / 16;  // 330 blocks: a tile of either kind at any phase
constexpr uint32_t kStage = kPad + kSpan + 2;               // and slack for the last window's 32-byte read
constexpr uint32_t kPer = (kSpan + kThreads - 1) / kThreads;
constexpr uint32_t kTrip = kThreads * 16;  // characters per trip of the scan, as the general decode (kern_b64.hpp)
constexpr uint32_t kSx = kTrip + 16;       // 4,096 + 3 sextets, whole 16-byte blocks
// The tile stages' two buffers and the scan's sextets are never live together.
constexpr uint32_t kStageBytes = 2 * kStage * 16;
static_assert(kSx <= kStageBytes, "the scan's sextets fit the tile buffers");

static_assert(sizeof(lbf_b64_state) == 16 && offsetof(lbf_b64_state, decoded) == 0 &&
                  offsetof(lbf_b64_state, carry) == 8 && offsetof(lbf_b64_state, ncarry) == 12 &&
                  offsetof(lbf_b64_state, ended) == 13 && offsetof(lbf_b64_state, zero) == 14,
              "lbf_b64_state layout");

using b64d::kEq;
using b64d::kSkip;
using b64d::pack16;
using b64d::six_groups;
using b64d::value;
// A tile's text staged behind kPad blocks (b64_device.hpp): LDS byte 16 * kPad + (src mod 16) + k = src[k].  The
// tile in hand decodes while the next one's text flies.
using Stage = b64d::Stage<kPer, kThreads, kPad>;

// Bytes [lo, hi) of the 16-byte block v to o[lo .. hi), with a plain store: the hash reads these bytes next.
__device__ __forceinline__ void put_block(uint8_t* o, uint4 v, uint32_t lo, uint32_t hi) {
  b64d::put_block<false>(o, 0u, lo, hi, v);
}

// A chain's record in registers, clamped: whatever a forged record says, the
// carry is at most three sextets and `decoded` at most 2^61.
struct Rec {
  uint64_t decoded;
  uint32_t carry, nc;
  bool ended;
};

__device__ __forceinline__ Rec read_rec(const uint8_t* rec) {
  const uint4 r = *reinterpret_cast<const uint4*>(rec);
  Rec s;
  s.decoded = (uint64_t)r.x | ((uint64_t)r.y << 32);
  if (s.decoded > kMaxDecoded) s.decoded = kMaxDecoded;  // forged: far past any slot, and it stays there
  s.nc = r.w & 3u;
  s.carry = r.z & ((1u << (6u * s.nc)) - 1u);
  s.ended = ((r.w >> 8) & 0xFFu) != 0;
  return s;
}

__device__ __forceinline__ uint4 rec_words(const Rec& s) {
  return make_uint4((uint32_t)s.decoded, (uint32_t)(s.decoded >> 32), s.carry, s.nc | (s.ended ? 0x100u : 0u));
}

// What a stage is given of a piece: the text it may take a prefix of, and the chunk's slot.
struct Piece {
  const uint8_t* t;
  uint32_t len;
  uint8_t* out;
  uint64_t slot;  // positions are sums of 64-bit numbers, taken mod 2^64
  uint32_t cap;
};

// The lane's block of a tile of lines: bytes [16 * lane, +16) of the tile from
// its six groups g0 .. g0 + 5 (kern_b64.hpp's b64_decode_block), of which only
// groups [gl, gh) of the tile are this piece's.  Character c of the tile is LDS
// byte delta + c.  *bad is set when one of the piece's groups holds a character
// outside the alphabet, or a separator place between two of its groups (up to
// group sep_hi - 1) holds one of the alphabet or '='.  Bytes of groups outside
// [gl, gh) are whatever lay in LDS; the caller stores none of them.
__device__ __forceinline__ uint4 decode_line_block(const uint8_t* sb, uint32_t delta, const uint8_t* tab, uint32_t gl,
                                                   uint32_t gh, uint32_t sep_hi, bool* bad) {
  const uint32_t b0 = 16 * threadIdx.x, g0 = b0 / 3, phase = b0 - 3 * g0;
  const uint32_t l0 = g0 / 18, r0 = g0 - 18 * l0;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(sb);
  const uint32_t c0 = delta + 4 * g0 + l0, sh0 = c0 & 3u;
  const uint32_t* wb = w + (c0 >> 2);
  uint32_t win[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) win[k] = wb[k];
  uint32_t x[6];
  uint32_t flags = 0;  // two bits per group, at 2j: zero exactly when its four characters are of the alphabet
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const uint32_t sep = r0 + j >= 18 ? 1u : 0u;
    const uint32_t off = sh0 + sep;  // 0..4: the group's offset from dword j of the window
    const uint32_t lo = off >= 4 ? win[j + 1] : win[j], hi = off >= 4 ? win[j + 2] : win[j + 1];
    const uint32_t c = __builtin_amdgcn_alignbyte(hi, lo, off & 3u);
    const uint32_t s0 = tab[c & 255], s1 = tab[(c >> 8) & 255], s2 = tab[(c >> 16) & 255], s3 = tab[c >> 24];
    flags |= ((s0 | s1 | s2 | s3) >> 6) << (2 * j);
    x[j] = (((s0 << 6) | s1) << 12) | ((s2 << 6) | s3);  // unmasked: a flagged group's bytes are never stored
  }
  const uint32_t jl = gl > g0 ? gl - g0 : 0u, jh = gh - g0 < 6u ? gh - g0 : 6u;  // g0 < gh, jl < 6: the caller's test
  const uint32_t mask = ((1u << (2 * jh)) - 1u) & ~((1u << (2 * jl)) - 1u);
  bool b = (flags & mask) != 0;
  if (r0 >= 12) {  // the line's separator follows window group 17 - r0
    const uint32_t js = 17 - r0, gs = g0 + js;
    if (gs >= gl && gs + 1 < sep_hi) b |= tab[sb[c0 + 4 * js + 4]] != kSkip;
  }
  *bad = b;
  return pack16(x, phase);
}

// The head of both tile stages: a carried group is completed from the piece's
// next 4 - nc characters.  Every lane works it out; lane 0 writes the three
// bytes (never at or past cap).  *D = the chain's byte count behind the head, a
// multiple of 3; *pos = the characters taken.  False when the piece is too
// short for the group or holds a character outside the alphabet there: the
// stage takes nothing.
__device__ __forceinline__ bool complete_carry(const Rec& r, const Piece& pc, uint64_t* D, uint32_t* pos) {
  *D = r.decoded;
  *pos = 0;
  if (r.nc == 0) return true;
  const uint32_t need = 4 - r.nc;
  if (pc.len < need) return false;
  uint32_t x = 0, junk = 0;
#pragma unroll
  for (uint32_t k = 0; k < 3; ++k)
    if (k < r.nc) x |= ((r.carry >> (6u * k)) & 63u) << (18u - 6u * k);
#pragma unroll
  for (uint32_t k = 1; k < 4; ++k) {
    if (k < r.nc) continue;
    const uint32_t v = value(pc.t[k - r.nc]);
    junk |= v >> 6;
    x |= (v & 63u) << (18u - 6u * k);
  }
  if (junk != 0) return false;
  if (threadIdx.x == 0) {
    uint8_t* const o = pc.out + (pc.slot + r.decoded);
    if (r.decoded < pc.cap) o[0] = (uint8_t)(x >> 16);
    if (r.decoded + 1 < pc.cap) o[1] = (uint8_t)(x >> 8);
    if (r.decoded + 2 < pc.cap) o[2] = (uint8_t)x;
  }
  *D = r.decoded + 3;  // at most 2^61 + 1: no wrap
  *pos = need;
  return true;
}

// The tile stages take nothing of a record the batch call would refuse (the data has ended, or `decoded` is no
// multiple of 3: forged) or of no text.  The same in every lane.
__device__ __forceinline__ bool nothing_to_take(const Rec& r, uint32_t len) {
  return r.ended || r.decoded % 3 != 0 || len == 0;
}

// A prefix that ends behind a group: the record moves on and nothing is carried.
__device__ __forceinline__ void move_on(Rec& r, uint64_t now) {
  if (now == r.decoded) return;  // a separator at the most: the record stays as it is
  r.decoded = now < kMaxDecoded ? now : kMaxDecoded;
  r.carry = 0;
  r.nc = 0;
}

// ---------------------------------------------------------------------------
// The line stage (b64_update_lines.hip has the rule): the longest prefix of
// the piece that continues xmlrpc++'s layout from where the record stands, the
// head by lane 0, then tiles of whole lines, each validated before it is
// stored.  Returns the characters taken and moves r on.  `tab` holds value() of
// every byte; the caller's barrier or the stage's first publishes it.  `peek`
// looks at the first separator place between two of the piece's groups before
// any tile is staged: a character of the alphabet or '=' there fails the first
// tile, which then takes nothing, so the stage stops behind the head as it
// would have after decoding that tile.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lines_stage(Rec& r, const Piece& pc, uint4 (*stage)[kStage], const uint8_t* tab,
                                                uint32_t (*wave_bad)[kWaves], bool peek) {
  if (nothing_to_take(r, pc.len)) return 0;  // the whole workgroup
  const uint8_t* const t = pc.t;
  const uint32_t len = pc.len, cap = pc.cap;
  uint64_t D;
  uint32_t pos;
  if (!complete_carry(r, pc, &D, &pos)) return 0;
  // ---- the separator at column 0, and the whole groups that follow by the piece's length
  const uint32_t col = (uint32_t)((D / 3) % 18);  // groups into the line
  bool sep_missing = false;
  if (col == 0 && pos < len) {
    if (value(t[pos]) == kSkip)
      ++pos;  // the separator, whether or not S is 0
    else
      sep_missing = r.nc != 0;  // the carried group ended a line: a separator follows it, or the piece's end
  }
  const uint32_t left = len - pos, n0 = 18 - col;  // n0 groups end the line in hand; then a separator and 72 a line
  uint32_t groups;
  if (sep_missing) {
    groups = 0;
  } else if (left < 4 * n0) {
    groups = left / 4;
  } else {
    const uint32_t more = left - 4 * n0, q = more / 73, rem = more - 73 * q;
    groups = n0 + 18 * q + (rem ? (rem - 1) / 4 : 0u);
  }
  if (groups) {  // '=' stops the prefix: only the last group of an encoder's text holds it
    const uint32_t k = groups - 1;
    const uint8_t* const g = t + pos + 4 * k + (k + col) / 18;
    if (g[0] == '=' || g[1] == '=' || g[2] == '=' || g[3] == '=') --groups;
  }
  // the separator behind the line in hand lies in the first tile, between two of the piece's groups
  if (peek && groups > n0 && value(t[pos + 4 * n0]) != kSkip) groups = 0;

  // ---- the tiles of the chunk that hold groups [D / 3, D / 3 + groups)
  uint32_t done = 0;  // groups of validated tiles
  if (groups) {
    const uint64_t tile0 = D / kTileBytes;
    const uint32_t g_first = (uint32_t)(D - tile0 * kTileBytes) / 3;  // the first group's index in its tile
    const uint32_t c_first = 4 * g_first + g_first / 18;              // and its first character's
    const uint32_t g_end = g_first + groups;                          // < 2^30 + 1,296
    const uint32_t ntiles = (g_end + kTileGroups - 1) / kTileGroups;
    Stage st;
    uint32_t delta_next = 0;
    // tile j's groups [gl, gh) and its characters [clo, chi): its groups', the separators between them, and the
    // one behind its last group when the next tile goes on
    auto load = [&](uint32_t j) {
      const uint32_t gl = j == 0 ? g_first : 0u;
      const uint32_t gh = g_end - j * kTileGroups < kTileGroups ? g_end - j * kTileGroups : kTileGroups;
      const uint32_t more = j + 1 < ntiles ? 1u : 0u;
      const uint32_t clo = 4 * gl + gl / 18, chi = 4 * gh + (gh - 1) / 18 + more;
      // piece character of tile character c: pos + (j * kLineTileText + c) - c_first
      const uint8_t* const src = t + pos + ((uint64_t)j * kLineTileText + clo - c_first);
      st.load(src, chi - clo);
      delta_next = 16 * kPad + (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u) - clo;  // mod 2^32
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
      if (mine)
        v = decode_line_block(reinterpret_cast<const uint8_t*>(stage[buf]), delta, tab, gl, gh, gh + (next ? 1u : 0u),
                              &bad);
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
      if (mine) {
        // the tile is good: the block's bytes that are the piece's and lie below cap
        const uint64_t tb = (tile0 + j) * kTileBytes;  // at most 2^61 + 3,888
        const uint32_t in_cap = cap > tb ? (cap - tb < kTileBytes ? (uint32_t)(cap - tb) : kTileBytes) : 0u;
        const uint32_t wlo = 3 * gl, whi = 3 * gh < in_cap ? 3 * gh : in_cap;
        if (whi > b0) put_block(pc.out + (pc.slot + tb + b0), v, wlo > b0 ? wlo - b0 : 0u, whi - b0);
      }
    }
  }
  // the characters behind `pos` that the done groups and the separators between them take
  const uint32_t taken = done ? pos + 4 * done + (done - 1 + col) / 18 : pos;
  move_on(r, D + 3ull * done);
  return taken;
}

// ---------------------------------------------------------------------------
// The flat stage (b64_flat.hip has the rule): the longest prefix of the text
// given that is unbroken -- the carried group completed, then whole groups of
// alphabet characters up to one that holds '=' -- a tile at a time, each
// validated before it is stored.  Returns the characters taken and moves r on.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t flat_stage(Rec& r, const Piece& pc, uint4 (*stage)[kStage], const uint8_t* tab,
                                               uint32_t (*wave_bad)[kWaves]) {
  if (nothing_to_take(r, pc.len)) return 0;  // the whole workgroup
  const uint8_t* const t = pc.t;
  const uint32_t len = pc.len, cap = pc.cap;
  uint64_t D;
  uint32_t pos;
  if (!complete_carry(r, pc, &D, &pos)) return 0;
  uint32_t groups = (len - pos) / 4;  // whole groups that follow, by the text's length
  if (groups) {                       // '=' stops the prefix: only the last group of a text holds it
    const uint8_t* const g = t + pos + 4 * (groups - 1);
    if (g[0] == '=' || g[1] == '=' || g[2] == '=' || g[3] == '=') --groups;
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
    // of the text
    auto load = [&](uint32_t j) {
      const uint32_t gl = j == 0 ? g_first : 0u;
      const uint32_t gh = g_end - j * kTileGroups < kTileGroups ? g_end - j * kTileGroups : kTileGroups;
      const uint8_t* const src = t + pos + ((uint64_t)j * kFlatTileText + 4 * gl - 4 * g_first);
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
      if (mine) {
        // the tile is good: the block's bytes that are the piece's and lie below cap
        const uint64_t tb = (tile0 + j) * kTileBytes;  // at most 2^61 + 3,888
        const uint32_t in_cap = cap > tb ? (cap - tb < kTileBytes ? (uint32_t)(cap - tb) : kTileBytes) : 0u;
        const uint32_t wlo = 3 * gl, whi = 3 * gh < in_cap ? 3 * gh : in_cap;
        if (whi > b0) put_block(pc.out + (pc.slot + tb + b0), v, wlo > b0 ? wlo - b0 : 0u, whi - b0);
      }
    }
  }
  move_on(r, D + 3ull * done);
  return pos + 4 * done;
}

// ---------------------------------------------------------------------------
// The general scan (b64_update.hip has the rule): the text given as arbitrary
// text, all of it, in trips of 4,096 characters.  The sextets of a trip go
// through LDS: sx[0, nc) holds the carried sextets, the trip's own follow, so
// group g of the trip is sx[4g, 4g + 4) and a lane's four groups are one
// aligned 16-byte LDS read.  On return r is the chain's record behind the
// text, in every lane.  The caller keeps other uses of sx's memory behind a
// barrier; the stage's own first barrier publishes `tab`.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void scan_stage(Rec& r, const Piece& pc, uint8_t* sx, const uint8_t* tab, uint32_t* sums,
                                           uint32_t* first_eq) {
  uint64_t decoded = r.decoded;
  uint32_t nc = r.nc;
  bool ended = r.ended;
  const uint32_t cap = pc.cap;
  if (threadIdx.x < 3) sx[threadIdx.x] = (uint8_t)((r.carry >> (6u * threadIdx.x)) & 63u);
  if (threadIdx.x == 0) *first_eq = 0xFFFFFFFFu;
  __syncthreads();

  const uint8_t* const t = pc.t;
  const uint64_t len = ended ? 0 : pc.len;
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
    uint32_t pos = nc + b64d::wg_exclusive_scan<kThreads>(cnt, sums, &total);
    // 4. sextets behind the carry; 5. the first '='.  pos < nc + 4,096 <= 4,099
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (c[k] == kSkip) continue;
      if (c[k] == kEq) atomicMin(first_eq, pos);
      sx[pos++] = c[k];
    }
    __syncthreads();
    // 6. complete groups before any '='
    const uint32_t m = nc + total, feq = *first_eq;
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
      uint8_t* const o = pc.out + (pc.slot + at_out);
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
        uint8_t* const o = pc.out + (pc.slot + at_end);
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
  uint32_t cw = 0;
  for (uint32_t k = 0; k < nc; ++k) cw |= (uint32_t)(sx[k] & 63u) << (6u * k);
  r.decoded = decoded;
  r.carry = cw;
  r.nc = nc;
  r.ended = ended;
}

// The piece's last step, by one lane: the piece table's entry for the bytes
// between `start` (the chain's byte count when the call began) and r, a final
// piece's length, and the record -- as lbf_b64_state_init leaves it behind a
// final piece (Final() restarts the chain; an unfinished group is dropped).
__device__ __forceinline__ void finish_piece(const Rec& r, uint64_t start, uint64_t slot, uint32_t cap, bool fin,
                                             uint8_t* rec, uint64_t* piece_off, uint32_t* piece_size,
                                             uint32_t* out_size) {
  const uint64_t before = start < cap ? start : (uint64_t)cap;
  const uint64_t after = r.decoded < cap ? r.decoded : (uint64_t)cap;
  *piece_off = slot + before;
  *piece_size = after > before ? (uint32_t)(after - before) : 0u;  // decoded never falls; checked all the same
  if (fin) *out_size = r.decoded <= cap ? (uint32_t)r.decoded : cap + 1u;
  *reinterpret_cast<uint4*>(rec) = fin ? make_uint4(0u, 0u, 0u, 0u) : rec_words(r);
}

}  // namespace b64s
}  // namespace lbf
