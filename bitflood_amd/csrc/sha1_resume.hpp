// sha1_resume.hpp -- what the resumable SHA-1 kernels share (sha1_update.hip:
// one piece per lane; sha1_update_seq.hip: one chain per lane): the layout of a
// caller-owned record (lbf_sha1_state, lbf_hash.h), its block as big-endian
// words, the closing compressions with a 64-bit length, and what a final piece
// writes.  The block loops are sha1_device.hpp's.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "lbf_hash.h"
#include "sha1_device.hpp"

namespace lbf {

constexpr uint32_t kStateBytes = 96, kBlockAt = 32;
static_assert(sizeof(lbf_sha1_state) == kStateBytes, "lbf_sha1_state is 96 bytes");
static_assert(offsetof(lbf_sha1_state, buffered) == 20 && offsetof(lbf_sha1_state, total) == 24 &&
                  offsetof(lbf_sha1_state, block) == kBlockAt,
              "lbf_sha1_state layout");

// The record's block as 16 big-endian words (four 16-byte loads: the block is
// at byte 32 of a 16-byte aligned record).
__device__ __forceinline__ void record_block(uint32_t (&w)[16], const uint8_t* blk) {
  const uint4* q = reinterpret_cast<const uint4*>(blk);
  const uint4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
  block_from_vec(w, q0, q1, q2, q3);
}

// Final one or two compressions from the r (< 64) bytes held in `w` (big-endian
// words of the record's block): 0x80 pad, zeros, and the bit length of `total`
// bytes as a 64-bit big-endian number in words 14-15 (iterhash.cpp:86-99,
// iterhash.h:30-31: GetBitCountHi = total >> 29, GetBitCountLo = total << 3).
__device__ __forceinline__ void finish64(Digest& s, uint32_t (&w)[16], uint32_t r, uint64_t total) {
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int rem = (int)r - 4 * k;  // message bytes left in this word
    uint32_t v = w[k];
    if (rem <= 0) v = 0;
    if (rem >= 0 && rem < 4) {
      const uint32_t sh = 8u * (uint32_t)rem;
      v = (v & ~(0xFFFFFFFFu >> sh)) | (0x80000000u >> sh);  // keep `rem` bytes, then 0x80
    }
    w[k] = v;
  }
  if (r >= 56) {
    compress(s, w);
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = 0;
  }
  w[14] = (uint32_t)(total >> 29);
  w[15] = (uint32_t)(total << 3);
  compress(s, w);
}

// What final piece i reports, into whichever of p.digests and p.verdicts (with
// p.expected) the launch has: the digest `be` holds as big-endian words.
template <class Params>
__device__ __forceinline__ void write_final(const Params& p, uint32_t i, const uint32_t (&be)[5]) {
  if (p.digests) {
    uint32_t* o = reinterpret_cast<uint32_t*>(p.digests + 20ull * i);
#pragma unroll
    for (int k = 0; k < 5; ++k) o[k] = be[k];
  }
  if (p.verdicts) {
    const uint32_t* e = reinterpret_cast<const uint32_t*>(p.expected + 20ull * i);
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) diff |= be[k] ^ e[k];
    p.verdicts[i] = diff == 0 ? 1 : 0;
  }
}

}  // namespace lbf
