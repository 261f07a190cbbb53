// b64_flat.hpp -- what wire_batch.cpp, b64_update.hip and update_batch.cpp
// need of the flat path of the base64 decode (b64_flat.hip): unbroken RFC 4648
// text, as bitflood's Java and Perl peers frame a chunk -- character i is
// sextet i, no line separators.  Two launchers (the one-shot pass of
// lbf_b64_verify_batch, the piecewise pass of lbf_b64_update_launch), the
// one-shot candidate test, and the process-wide switch.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b64_encode_update.hpp"
#include "lbf_hash.h"

namespace lbf {

// A chunk of `cap` bytes that arrives as `text_len` characters is a candidate
// for the one-shot flat pass when the length is the unbroken text's and not
// the encoder's.  Chunks of 54 bytes or less stay with the one-pass decode: up
// to 53 bytes the two layouts are one text, and the 72 characters of 54 bytes
// are a line the one-pass decode takes without its trailing separator.
// (b64e::text_length(cap, false) is lbf_b64_put_length(cap); host and device: b64_decode_routed_kernel routes by it.)
LBF_ENC_HD inline bool b64_flat_candidate(uint32_t text_len, uint32_t cap) {
  return cap > 54 && text_len == 4 * (((uint64_t)cap + 2) / 3) && text_len != b64e::text_length(cap, false);
}

// b64_flat_decode_kernel's arrays: those of the one-pass decode (B64Launch,
// lbf_internal.hpp).  The pass takes chunks [chunk0, chunk0 + n), every one a
// candidate; a chunk whose text is not flat is marked in redo[] and left to
// the general decode.
struct B64FlatDecode {
  const uint8_t* text;
  const uint64_t* text_off;
  const uint32_t* text_len;
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* cap;
  uint32_t* sizes;
  uint8_t* over;
  uint8_t* redo;
  uint32_t chunk0;
  uint32_t n;
  uint32_t max_text_len;  // of the n chunks: the tiles per chunk
};
int launch_b64_flat_decode(const B64FlatDecode& b, hipStream_t stream);

// b64_update_flat_kernel's parameters: lbf_b64_update_launch's arrays.  The two
// work arrays carry the hand-off to b64_update_kernel, as the line path's do
// (b64_update_lines.hpp): before[i] = the chain's byte count when the call
// began, taken[i] = the characters of piece i already decoded.  With
// after_lines the line kernel has written both and moved the record on: the
// flat kernel starts behind taken[i], adds what it takes and leaves before[i].
struct B64FlatParams {
  uint8_t* b64_states;
  uint64_t n_states;
  const uint32_t* state_of;
  const uint8_t* text;
  const uint64_t* text_off;
  const uint32_t* text_len;
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* cap;
  uint64_t* before;      // d_piece_offsets
  uint32_t* taken;       // d_piece_sizes
  uint32_t* flat_chars;  // null, or n entries that receive the characters this kernel took (skipped pieces' stay)
  uint32_t after_lines;
};

// One workgroup per piece, on `stream`.
int launch_b64_update_flat(const B64FlatParams& p, uint32_t n, hipStream_t stream);

// lbf_set_b64_flat's current value; before the first call or setter,
// LBF_B64_FLAT ("0" switches a default-on path off, "1" a default-off one on).
// Off: behind the line path the extra enqueue costs encoder-layout text 0.05 ms
// per 4 GiB at 64 KiB pieces and 0.63 ms at 4 KiB pieces, more than the rounds
// spread; a receiver with Java or Perl peers switches it on.
constexpr bool kB64FlatDefault = false;
bool b64_flat_enabled();

}  // namespace lbf
