// b64_update_lines.hpp -- what b64_update.hip and update_batch.cpp need of
// the line path of the piecewise decode (b64_update_lines.hip): its launcher,
// the process-wide switch, and the launch that also reports, per piece, the
// characters the line path took.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lbf_hash.h"

namespace lbf {

// b64_update_lines_kernel's parameters: lbf_b64_update_launch's arrays.  The
// two work arrays carry the hand-off to b64_update_kernel: before[i] = the
// chain's byte count when the call began (clamped as the kernels clamp it),
// taken[i] = the characters of piece i the line path decoded.
struct B64LinesParams {
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
  uint32_t* line_chars;  // null, or n entries that receive taken[i] (entries of skipped pieces stay)
};

// One workgroup per piece, on `stream`.
int launch_b64_update_lines(const B64LinesParams& p, uint32_t n, hipStream_t stream);

// lbf_set_b64_lines's current value; before the first call or setter,
// LBF_B64_LINES ("0" switches a default-on path off, "1" a default-off one on).
constexpr bool kB64LinesDefault = true;
bool b64_lines_enabled();

// lbf_b64_update_launch with two more device arrays (each null, or n entries,
// zero on entry): the characters of each piece that went through the line
// path, and those the flat path (b64_flat.hip) took of what it left.
int b64_update_launch_counted(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                              const uint32_t* d_state_of, const char* d_text, const uint64_t* d_text_offsets,
                              const uint32_t* d_text_lens, const uint8_t* d_final, uint64_t n, uint8_t* d_out,
                              const uint64_t* d_out_offsets, const uint32_t* d_caps, uint32_t* d_out_sizes,
                              uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                              uint64_t* d_piece_offsets, uint32_t* d_piece_sizes, uint32_t* d_line_chars,
                              uint32_t* d_flat_chars, void* stream);

// lbf_b64_update_seq_launch with two more device arrays (each null, or n
// entries): the characters of each piece that the line stage and the flat
// stage took, as b64_update_launch_counted reports them.
int b64_update_seq_launch_counted(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                  const uint32_t* d_chain_state, const uint32_t* d_chain_first, uint64_t n_chains,
                                  const char* d_text, const uint64_t* d_text_offsets, const uint32_t* d_text_lens,
                                  const uint8_t* d_final, uint64_t n, uint8_t* d_out, const uint64_t* d_out_offsets,
                                  const uint32_t* d_caps, uint32_t* d_out_sizes, uint8_t* d_digests,
                                  const uint8_t* d_expected, uint8_t* d_verdicts, uint64_t* d_piece_offsets,
                                  uint32_t* d_piece_sizes, uint32_t* d_line_chars, uint32_t* d_flat_chars,
                                  void* stream);

}  // namespace lbf
