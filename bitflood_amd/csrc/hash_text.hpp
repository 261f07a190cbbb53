// hash_text.hpp -- the geometry and the work layout of lbf_sha1_hashes_launch
// and lbf_verify_hashes_launch (hash_text.hip): chunks resident in device
// memory to and against the flood file's 27-character hash strings, chunkmap
// and to-download list built on the device.  Not part of the ABI.
// DESIGN.md §4.10.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lbf_hash.h"

namespace lbf {
namespace htext {

// A hash string: the unpadded base64 of a 20-byte digest (Encoder.cpp:104-105).
constexpr uint32_t kHashChars = 27;
// hash_text_encode_kernel: chunks (lanes) a workgroup.
constexpr uint32_t kEncBlock = 256;
// hash_text_compare_kernel / hash_text_scatter_kernel: chunks (lanes) a
// workgroup, 16 waves; one count of '0' per workgroup goes to the work area.
constexpr uint32_t kMapBlock = 1024;
// hash_text_scan_kernel: the lanes of its one workgroup, and the counts it
// takes a trip.
constexpr uint32_t kScanWidth = 1024;

// d_work: [0, 20 n) the digests when the caller gives none, then from the next
// multiple of 16 one uint32 per workgroup of the compare kernel (its count of
// '0', turned into the workgroup's base in the list by the scan kernel).
constexpr uint64_t map_blocks(uint64_t n) { return (n + kMapBlock - 1) / kMapBlock; }
constexpr uint64_t counts_at(uint64_t n) { return (20 * n + 15) & ~15ull; }
constexpr uint64_t work_bytes(uint64_t n) { return counts_at(n) + 4 * map_blocks(n); }

// The tables of one verify launch, all device memory.
struct HashTextVerify {
  const uint8_t* digests;    // n x 20, written by the hash in front
  const uint8_t* hashes;
  const uint64_t* hash_off;  // null (with hash_len): packed, 27 * i
  const uint32_t* hash_len;
  uint8_t* chunkmap;         // n characters, '1' / '0'
  uint32_t* counts;          // map_blocks(n) words of d_work; null with missing
  uint32_t* missing;         // null, or room for n indices
  uint32_t* missing_count;
  uint32_t n;
};

// digests -> strings at hashes + hash_off[i], or + 27 * i when hash_off is null.
int launch_hash_text_encode(const uint8_t* digests, uint8_t* hashes, const uint64_t* hash_off, uint32_t n,
                            hipStream_t stream);
// compare (chunkmap, counts), then scan and scatter when v.missing is given.
int launch_hash_text_verify(const HashTextVerify& v, hipStream_t stream);

}  // namespace htext
}  // namespace lbf
