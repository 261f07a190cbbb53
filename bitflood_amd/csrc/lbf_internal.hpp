// lbf_internal.hpp -- shared internals of liblbfhash.so (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>

#include "lbf_hash.h"

namespace lbf {

// Thread-local last-error slot behind lbf_last_error().
void set_error(const std::string& msg);
int fail(int status, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define LBF_HIP_TRY(expr)                                   \
  do {                                                      \
    hipError_t lbf_e_ = (expr);                             \
    if (lbf_e_ != hipSuccess) return ::lbf::hip_fail(lbf_e_, #expr); \
  } while (0)

// Kernel-side parameter block shared by every chunk-hash kernel variant.
struct ChunkParams {
  const uint8_t* base;
  const uint64_t* offsets;   // null => uniform chunking of [0, len)
  const uint32_t* sizes;
  uint64_t len;              // uniform: region length
  uint64_t first_chunk;      // uniform: index of chunk 0 of this launch
  uint32_t chunk_size;       // uniform
  uint32_t n;                // chunks in this launch
  uint8_t* digests;          // n*20 bytes or null
  const uint8_t* expected;   // n*20 bytes or null
  uint8_t* verdicts;         // n bytes or null
};

// A device array the caller passed must fit in the allocation it points into
// (sha1_kernels.hip); LBF_OK for null, empty, or memory HIP cannot place.
int check_fits(const void* p, uint64_t bytes, const char* what);

// One device array of a launch: `count` elements of `elem` bytes, by the name
// the refusals use; `aligned` when the launch needs it aligned to its element.
struct DevTable {
  const void* p;
  uint64_t elem, count;
  const char* name;
  bool aligned;
};

// The device launches' validator, in two passes that a launch may put refusals
// of its own between: one refusal for the whole list when an array that needs
// it is not aligned to its element size, then check_fits per array in list
// order, named "<who>: <name>".
inline int tables_aligned(const std::string& who, std::initializer_list<DevTable> tables) {
  for (const DevTable& t : tables)
    if (t.aligned && reinterpret_cast<uintptr_t>(t.p) % t.elem)
      return fail(LBF_ERR_INVALID, who + ": a table is not aligned to its element size");
  return LBF_OK;
}

inline int tables_fit(const std::string& who, std::initializer_list<DevTable> tables) {
  for (const DevTable& t : tables)
    if (int rc = check_fits(t.p, t.elem * t.count, (who + ": " + t.name).c_str())) return rc;
  return LBF_OK;
}

int pick_variant(uint64_t n);
int launch_chunks(const ChunkParams& p, hipStream_t stream);

// Device base64 decode (kern_b64.hpp): n chunks' text -> bytes, on `stream`.
struct B64Launch {
  const uint8_t* text;
  uint8_t* scratch;
  const uint64_t* text_off;
  const uint64_t* sext_off;
  const uint32_t* text_len;
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* cap;
  uint32_t* sizes;
  uint8_t* over;
  uint8_t* redo;  // n bytes, zero on entry: the chunks the one-pass decode hands to the general one
  uint32_t n;
  uint32_t max_text_len;  // the longest text and the largest cap: the one-pass decode's tiles per chunk
  uint32_t max_cap;
};
int launch_b64_decode(const B64Launch& b, hipStream_t stream);
// Its two halves, for a caller that puts another pass between them (wire_batch.cpp: the flat pass of b64_flat.hip
// marks redo[] too): the one-pass decode of the first b.n chunks, the general decode of those redo[] names.
int launch_b64_decode_one_pass(const B64Launch& b, hipStream_t stream);
int launch_b64_decode_general(const B64Launch& b, hipStream_t stream);
// Device base64 encode (kern_b64.hpp): n chunks' bytes -> their SendChunk text.
// max_size: the largest chunk (sets the tiles per chunk).
int launch_b64_encode(const uint8_t* data, const uint64_t* data_off, const uint32_t* size, uint8_t* text,
                      const uint64_t* text_off, uint32_t n, uint32_t max_size, hipStream_t stream);

// Kernel variants beyond the shipped ones (1, 7, 10, 11, 12).  Null in the
// shipped library; the A/B library of tools/experimental/ points it at its
// superseded and diagnostic variants when it loads.
struct ExtraVariants {
  bool (*known)(int variant);
  bool (*launch)(int variant, const ChunkParams& p, hipStream_t stream);
};
extern const ExtraVariants* g_extra_variants;

}  // namespace lbf
