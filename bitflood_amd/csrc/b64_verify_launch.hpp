// b64_verify_launch.hpp -- the arrays and the geometry of
// lbf_b64_verify_launch (b64_verify_launch.hip): the receiver's one-shot
// decode + verify for chunk text that is resident in device memory, every
// decision that lbf_b64_verify_batch makes on the host made on the device.
// Not part of the ABI.  DESIGN.md §4.5.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_encode_update.hpp"
#include "lbf_hash.h"

namespace lbf {

// The bounds the launch takes: a chunk of at most 1 GiB from at most 1.5 GiB
// of text, as lbf_b64_verify_batch (the kernels keep positions in 32 bits).
constexpr uint64_t kVerifyLaunchMaxSize = b64e::kEncMaxChunk, kVerifyLaunchMaxText = 3ull << 29;

// The tables of one launch, all device memory.  sizes/over/redo are written by
// the decode kernels under the one-pass decode's contract (kern_b64.hpp):
// sizes[i] = min(decoded, cap[i]), over[i] = decoded > cap[i], redo[i] = 1 for
// a chunk the tile pass handed to the scan.  b64_verify_finish_kernel then
// turns sizes[] into the public d_out_sizes.
struct B64VerifyLaunch {
  const uint8_t* text;
  const uint64_t* text_off;
  const uint32_t* text_len;
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* cap;  // d_expected_sizes
  uint32_t* sizes;      // d_out_sizes
  uint8_t* over;        // d_work[0, n)
  uint8_t* redo;        // d_work[n, 2n)
  uint8_t* verdicts;    // null, or what the hash wrote
  uint32_t n;
  uint32_t max_text_len, max_size;  // a chunk over either is not decoded
};

// The enqueues between the memset of d_work and the hash (routed tile pass,
// scan of the redo chunks), and the one behind it (sizes and verdicts).
int launch_b64_verify_decode(const B64VerifyLaunch& b, hipStream_t stream);
int launch_b64_verify_finish(const B64VerifyLaunch& b, hipStream_t stream);

}  // namespace lbf
