// b64_device.hpp -- the device helpers of every base64 kernel (gfx950), each
// stated once: the staging of a span through registers into LDS, the clipped
// 16-byte block store, the decode table entry and the alphabet, the workgroup
// scan, a group's characters, a lane's six groups from a window of unbroken
// text, and the packing of six groups' bytes into a 16-byte block.
//
// Every function is __device__ __forceinline__ and the header defines no
// kernel, no __constant__ and no __shared__: including it adds no symbol to a
// translation unit and no instruction to a kernel that does not call it.  The
// kernels of kern_b64.hpp (in sha1_kernels.hip), b64_update_stages.hpp,
// b64_flat.hip, b64_encode_update.hip and b64_flat_encode.hip are built from
// these; where they differ the difference is a parameter, and the comment says
// which kernel sets it how.  Their instruction streams are pinned by
// tests/golden/isa_shipped.json and tests/golden/isa_b64.json (tests/test_isa.py):
// moving a helper here left every kernel's stream as it was.  Two did not move,
// because as functions they change the streams of their kernels: the six-group
// window of a tile of LINES (kern_b64.hpp's b64_decode_block, with its A/B
// form, and b64_update_stages.hpp's decode_line_block) and the five-word block
// of a line's text (kern_b64.hpp's b64_encode_tile, b64_encode_update.hip's
// enc_tile).
//
// The lane number is threadIdx.x as the including translation unit defines it
// (b64_update_seq.hip reads it through a wrapper of its own).  Nothing here
// synchronises but __syncthreads(), and no function leaves early in some lanes
// only in front of one.  DESIGN.md §4.5, §4.7, §4.8.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lbf {
namespace b64d {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // what the nontemporal builtins take

// Decode table entries: 0..63 for the alphabet, kEq for '=', kSkip otherwise.
constexpr uint32_t kEq = 64, kSkip = 255;

// The decode table entry of character c, computed: filling an LDS copy this way
// costs a few VALU per lane and no dependent global load.
__device__ __forceinline__ uint32_t value(uint32_t c) {
  return c - 'A' < 26u ? c - 'A' : c - 'a' < 26u ? c - 'a' + 26 : c - '0' < 10u ? c - '0' + 52 :
         c == '+' ? 62u : c == '/' ? 63u : c == '=' ? kEq : kSkip;
}

// The alphabet into 64 bytes of LDS, by the first 64 lanes; the caller's next
// barrier publishes it.
__device__ __forceinline__ void fill_alphabet(uint8_t* alpha) {
  if (threadIdx.x < 64) {
    const uint32_t c = threadIdx.x;
    alpha[c] = (uint8_t)(c < 26 ? 'A' + c : c < 52 ? 'a' + (c - 26) : c < 62 ? '0' + (c - 52) : c == 62 ? '+' : '/');
  }
}

// Four bytes of LDS from any byte address (two aligned dword reads + v_alignbyte).
__device__ __forceinline__ uint32_t lds_u32_at(const uint32_t* w, uint32_t at) {
  return __builtin_amdgcn_alignbyte(w[(at >> 2) + 1], w[at >> 2], at & 3u);
}

// Exclusive scan of one value per lane over a workgroup of kThreads lanes;
// returns the lane's prefix and writes the total to *total.  `sums` is
// kThreads / 64 words of LDS, free again when the call returns.
template <uint32_t kThreads>
__device__ __forceinline__ uint32_t wg_exclusive_scan(uint32_t v, uint32_t* sums, uint32_t* total) {
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
  for (int w = 0; w < (int)(kThreads / 64); ++w) {
    const uint32_t s = sums[w];
    before += w < wave ? s : 0u;
    all += s;
  }
  __syncthreads();  // sums is reused by the next call
  *total = all;
  return before + x - v;
}

// Stage global bytes [src, src + len) in LDS as the aligned 16-byte blocks that
// hold them, behind kFrontBlocks blocks the caller keeps for itself: afterwards
// LDS byte 16 * kFrontBlocks + delta + k = src[k], delta = src mod 16.  The
// blocks are read whole (a 16-byte block holding one byte of the span lies in
// the same page, so this never reads an unmapped address), up to kPer per lane
// of kThreads.  load() issues all of a lane's loads and returns at once;
// store() waits for them and writes LDS, so work placed between the two (the
// table, the tile in hand) runs while the loads are in flight.
//   kFrontBlocks: 0 in the one-shot kernels; 2 in the piecewise decode, whose
//   first window starts up to 24 characters in front of the piece; 1 in the
//   piecewise encode, for the carried bytes below the piece's first.
template <uint32_t kPer, uint32_t kThreads, uint32_t kFrontBlocks>
struct Stage {
  u32x4 v[kPer];
  uint32_t blocks = 0, delta = 0;
  __device__ __forceinline__ void load(const uint8_t* src, uint32_t len) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    delta = (uint32_t)(a & 15u);
    const u32x4* g = reinterpret_cast<const u32x4*>(a - delta);
    blocks = (delta + len + 15) / 16;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (threadIdx.x + k * kThreads < blocks) v[k] = __builtin_nontemporal_load(g + threadIdx.x + k * kThreads);
  }
  // No span: store() writes nothing.  A caller whose span may be empty clears
  // and then loads only if it is not (its address may be the end of an allocation).
  __device__ __forceinline__ void clear() {
    blocks = 0;
    delta = 0;
  }
  __device__ __forceinline__ void store(uint4* lds) const {
    u32x4* l = reinterpret_cast<u32x4*>(lds) + kFrontBlocks;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (threadIdx.x + k * kThreads < blocks) l[threadIdx.x + k * kThreads] = v[k];
  }
};

// The 16-byte block v at base + pos, clipped to positions [lo, hi): one 16-byte
// store when it lies wholly inside and its address is aligned, bytes otherwise.
// Nothing outside [lo, hi) is written.
//   Pos: 64-bit in the one-shot line kernels (kern_b64.hpp), 32-bit elsewhere.
//   kNontemporal: the store kind; all but the piecewise decode's stages, whose
//   bytes the hash reads next, stream past the cache.
//   kEarlyExit: the byte tail as a loop that stops at hi (kern_b64.hpp, whose
//   recorded code has that form) in place of sixteen predicated stores.
template <bool kNontemporal = true, bool kEarlyExit = false, typename Pos>
__device__ __forceinline__ void put_block(uint8_t* base, Pos pos, Pos lo, Pos hi, uint4 v) {
  uint8_t* dst = base + pos;
  if (pos >= lo && pos + 16 <= hi && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0) {
    if constexpr (kNontemporal) {
      const u32x4 x = {v.x, v.y, v.z, v.w};
      __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst));
    } else {
      *reinterpret_cast<uint4*>(dst) = v;
    }
    return;
  }
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  if constexpr (kEarlyExit) {
    for (uint32_t m = 0; m < 16 && pos + m < hi; ++m)
      if (pos + m >= lo) dst[m] = (uint8_t)(w[m >> 2] >> (8 * (m & 3)));
  } else {
#pragma unroll
    for (uint32_t m = 0; m < 16; ++m)
      if (pos + m >= lo && pos + m < hi) dst[m] = (uint8_t)(w[m >> 2] >> (8 * (m & 3)));
  }
}

// ---------------------------------------------------------------------------
// Encode: bytes in LDS -> characters.
// ---------------------------------------------------------------------------
// The three bytes of a group at LDS byte `at`, first byte highest, as 24 bits.
__device__ __forceinline__ uint32_t group_bits(const uint32_t* w, uint32_t at) {
  return __builtin_amdgcn_perm(0u, lds_u32_at(w, at), 0x0C000102u);
}

// A whole group's 24 bits as its four characters, first character in the low byte.
__device__ __forceinline__ uint32_t chars_whole(const uint8_t* alpha, uint32_t x) {
  return (uint32_t)alpha[x >> 18] | (uint32_t)alpha[(x >> 12) & 63] << 8 | (uint32_t)alpha[(x >> 6) & 63] << 16 |
         (uint32_t)alpha[x & 63] << 24;
}

// The last group of a chunk of `rest` (1 or 2) bytes over: "xx==" / "xxx=".
__device__ __forceinline__ uint32_t chars_last(const uint8_t* alpha, uint32_t x, uint32_t rest) {
  x &= rest == 2 ? 0xFFFF00u : 0xFF0000u;
  return (uint32_t)alpha[x >> 18] | (uint32_t)alpha[(x >> 12) & 63] << 8 |
         (rest == 2 ? (uint32_t)alpha[(x >> 6) & 63] : (uint32_t)'=') << 16 | (uint32_t)'=' << 24;
}

// ---------------------------------------------------------------------------
// Decode: characters in LDS -> bytes.  `tab` is value() of every byte, in LDS.
// A lane's block, bytes [16u, 16u + 16) of a tile, comes from the six groups
// g0 = 16u / 3 onwards.
// ---------------------------------------------------------------------------
// The six groups of unbroken text from LDS bytes [c0, c0 + 24): one window of
// seven aligned dwords, each group cut out of it with v_alignbyte.  x[j] =
// group j's 24 bits, joined unmasked: an entry above 63 spoils only its own
// group's bytes, and the callers store no such group's bytes as data.  (entry
// >> 6) is 0 exactly for an alphabet character: two flag bits per group at 2j,
// for all four characters (*inner) and for the first two (*head).  Groups past
// the text are decoded from whatever lies in LDS; the callers mask their flags
// and cut their bytes.
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

// Bytes [phase, phase + 16) of six groups' 18: group j's bytes are x[j]'s
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

}  // namespace b64d
}  // namespace lbf
