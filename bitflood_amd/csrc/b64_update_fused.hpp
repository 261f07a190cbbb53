// b64_update_fused.hpp -- what b64_update.hip needs of the fused route of the
// piecewise decode (b64_update_fused.hip): one kernel that runs the line stage,
// the flat stage and the general scan of a piece in one launch, its launcher,
// and the process-wide switch.  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lbf_hash.h"

namespace lbf {

// b64_update_fused_kernel's parameters: lbf_b64_update_launch's arrays, as the
// three stage kernels get them.  piece_off / piece_size are written once, with
// their final values.
struct B64FusedParams {
  uint8_t* b64_states;  // n_states records of 16 bytes, 16-byte aligned
  uint64_t n_states;
  const uint32_t* state_of;  // chain of each piece, or null: piece i -> chain i
  const uint8_t* text;
  const uint64_t* text_off;
  const uint32_t* text_len;
  const uint8_t* final_flags;  // null => no piece is final
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* cap;
  uint32_t* out_sizes;  // written for final pieces only
  uint64_t* piece_off;  // the table lbf_sha1_update_launch reads
  uint32_t* piece_size;
  uint32_t* line_chars;  // null, or n entries: the characters the line stage took (written when it is on)
  uint32_t* flat_chars;  // null, or n entries: the characters the flat stage took (written when it is on)
  uint32_t stages;       // kB64StageLines | kB64StageFlat: the stages in front of the scan
};
constexpr uint32_t kB64StageLines = 1, kB64StageFlat = 2;

// One workgroup per piece, on `stream`.
int launch_b64_update_fused(const B64FusedParams& p, uint32_t n, hipStream_t stream);

// lbf_set_b64_fused's current value; before the first call or setter,
// LBF_B64_FUSED ("1" switches it on).  Off: the default route's enqueues stay
// as they were, and switching it on is a step of its own.
constexpr bool kB64FusedDefault = false;
bool b64_fused_enabled();

}  // namespace lbf
