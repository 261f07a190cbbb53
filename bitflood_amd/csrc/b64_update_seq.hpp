// b64_update_seq.hpp -- what the host batch call needs of b64_update_seq.hip
// beyond the ABI.  Not part of the ABI.
#pragma once

#include <stdint.h>

#include "lbf_hash.h"

namespace lbf {

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
