// b64_encode_update.hpp -- the geometry of a chunk's base64 text, stated once
// for every wire call: xmlrpc++'s line, where a group's characters lie in
// either peer layout, how long the text is, and the wire calls' bound on a
// chunk; and the tile the kernel of b64_encode_update.hip (the resumable
// encode, lbf_b64_enc_state, lbf_hash.h) lays over it.  Plain constexpr
// arithmetic, no HIP: the kernels, the launches and the batch calls' planners
// all read the rule from here, and tests/test_b64_encode_cpu.py reads the
// constants back.  DESIGN.md §4.8.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LBF_ENC_HD __host__ __device__
#else
#define LBF_ENC_HD
#endif

namespace lbf {
namespace b64e {

// xmlrpc++'s line: 18 groups, 54 bytes, 72 characters and the separator.
constexpr uint32_t kLineGroups = 18, kLineBytes = 54, kLineChars = 73;
constexpr uint8_t kSeparator = ' ';

// The tile: whole lines of the CHUNK's text, so that a 16-byte block of text
// falls at the same place however the chunk is cut.  112 lines as the one-shot
// encode's (kern_b64.hpp): 6,048 bytes -> 8,176 characters in lines (511
// blocks, two per lane), 8,064 unbroken (504 blocks).  Bytes and both texts of a
// tile are whole 16-byte blocks: a multiple of 16 lines.
constexpr uint32_t kEncUpdLines = 112;
constexpr uint32_t kEncUpdTileGroups = kEncUpdLines * kLineGroups;  // 2,016 groups
constexpr uint32_t kEncUpdTileBytes = kEncUpdLines * kLineBytes;    // 6,048 bytes
constexpr uint32_t kEncUpdTileText = kEncUpdLines * kLineChars;     // 8,176 characters in lines
constexpr uint32_t kEncUpdTileFlat = kEncUpdTileGroups * 4;         // 8,064 characters unbroken
constexpr uint32_t kEncUpdThreads = 256;
static_assert(kEncUpdTileBytes % 16 == 0 && kEncUpdTileText % 16 == 0 && kEncUpdTileFlat % 16 == 0,
              "tiles of 16-byte blocks");

// P(G): the text position of group G.
LBF_ENC_HD constexpr uint64_t group_pos(uint64_t g, bool flat) { return flat ? 4 * g : 4 * g + g / kLineGroups; }
// T(n): the length of the text of n bytes.
LBF_ENC_HD constexpr uint64_t text_length(uint64_t n, bool flat) {
  return group_pos(n / 3, flat) + (n % 3 ? 4 : 0);
}

// The wire calls' bound on a chunk, encode and decode, one-shot and piecewise
// (1 GiB), and the longest text such a chunk has: the kernels keep positions
// within a chunk and its text in 32 bits.
constexpr uint64_t kEncMaxChunk = 1ull << 30;
constexpr uint64_t kEncMaxTextCap = text_length(kEncMaxChunk, false);  // 1,451,539,875
static_assert(kEncMaxTextCap + kEncUpdTileText < (1ull << 32), "text positions fit 32 bits");
// A chain's byte count stays below this (the SHA-1 bit count is a 64-bit number).
constexpr uint64_t kEncMaxTaken = 1ull << 61;

}  // namespace b64e
}  // namespace lbf
