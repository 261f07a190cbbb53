// sha1_update.hip -- resumable SHA-1 on the GPU: one piece of a chunk per lane,
// absorbed into a caller-owned 96-byte state (lbf_sha1_state, lbf_hash.h).
//
// The reference's hash object takes Update() calls of any length and then
// Final(), which restarts it (Crypto++ 5.2.1 IteratedHash, iterhash.cpp:9-99,
// iterhash.h:120); the one-shot kernels of sha1_kernels.hip need a chunk's
// bytes in one range.  Here a launch continues each chain from its record:
// top up the buffered block, run the full blocks straight from the piece (the
// lane kernel's loops, sha1_device.hpp), keep the last < 64 bytes in the record,
// and on a piece flagged final pad with the 64-bit length, write the digest
// and/or verdict, and put the record back to its initial value.
//
// A translation unit of its own: it is no kernel "variant" (lbf_kernel_for and
// lbf_set_kernel_variant do not know it).  What it shares with
// sha1_update_seq.hip is sha1_resume.hpp.  DESIGN.md §4.6.
#include <hip/hip_runtime.h>

#include "lbf_internal.hpp"
#include "sha1_resume.hpp"

namespace lbf {

namespace {

struct UpdateParams {
  uint8_t* states;            // n_states records of 96 bytes, 16-byte aligned
  uint64_t n_states;
  const uint32_t* state_of;   // state of each piece, or null: piece i -> state i
  const uint8_t* base;
  const uint64_t* offsets;
  const uint32_t* sizes;
  const uint8_t* final_flags; // null => no piece is final
  uint32_t n;
  uint8_t* digests;           // n*20 or null; written for final pieces only
  const uint8_t* expected;    // n*20 or null
  uint8_t* verdicts;          // n or null; written for final pieces only
};

__global__ void __launch_bounds__(256) sha1_update_kernel(UpdateParams p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no state: nothing is read or written for it
  uint8_t* const rec = p.states + kStateBytes * si;
  uint8_t* const blk = rec + kBlockAt;

  const uint4 lo = reinterpret_cast<const uint4*>(rec)[0];  // h[0..3]
  const uint4 hi = reinterpret_cast<const uint4*>(rec)[1];  // h[4], buffered, total
  Digest s;
  s.h[0] = lo.x; s.h[1] = lo.y; s.h[2] = lo.z; s.h[3] = lo.w; s.h[4] = hi.x;
  // & 63: whatever a forged record says, every byte index below stays inside
  // the record's own 64-byte block
  uint32_t buf = hi.y & 63u;
  uint64_t total = (uint64_t)hi.z | ((uint64_t)hi.w << 32);

  const uint8_t* src = p.base + p.offsets[i];
  uint32_t size = p.sizes[i];
  const bool fin = p.final_flags != nullptr && p.final_flags[i] != 0;
  total += size;

  if (buf) {
    // Top the unfinished block up in the record itself and read it back whole:
    // a register array indexed by `buf` would live in scratch.
    const uint32_t room = 64u - buf;
    const uint32_t take = size < room ? size : room;
    for (uint32_t k = 0; k < take; ++k) blk[(buf + k) & 63u] = src[k];
    src += take;
    size -= take;
    buf += take;
    if (buf == 64u) {
      uint32_t w[16];
      record_block(w, blk);
      compress(s, w);
      buf = 0;
    }
  }
  // here buf == 0, or the piece is used up (size == 0)
  const uint32_t nblk = size >> 6;
  if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    hash_blocks_aligned(s, src, nblk);
  } else {
    hash_blocks_unaligned(s, src, nblk);
  }
  src += 64ull * nblk;
  const uint32_t rem = size & 63u;  // non-zero only with buf == 0
  for (uint32_t k = 0; k < rem; ++k) blk[(buf + k) & 63u] = src[k];
  buf = (buf + rem) & 63u;

  uint4* const out = reinterpret_cast<uint4*>(rec);
  if (!fin) {
    out[0] = make_uint4(s.h[0], s.h[1], s.h[2], s.h[3]);
    out[1] = make_uint4(s.h[4], buf, (uint32_t)total, (uint32_t)(total >> 32));
    return;
  }

  uint32_t w[16];
  record_block(w, blk);
  finish64(s, w, buf, total);
  uint32_t be[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) be[k] = bswap(s.h[k]);  // digest bytes in big-endian order
  write_final(p, i, be);
  // Final() restarts the object (iterhash.h:120): the record is as
  // lbf_sha1_state_init leaves it
  out[0] = make_uint4(kH0, kH1, kH2, kH3);
  out[1] = make_uint4(kH4, 0u, 0u, 0u);
#pragma unroll
  for (int k = 2; k < 6; ++k) out[k] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

}  // namespace lbf

using lbf::fail;

extern "C" void lbf_sha1_state_init(lbf_sha1_state* states, uint64_t n) {
  if (!states) return;
  for (uint64_t k = 0; k < n; ++k) {
    lbf_sha1_state& s = states[k];
    s.h[0] = lbf::kH0; s.h[1] = lbf::kH1; s.h[2] = lbf::kH2; s.h[3] = lbf::kH3; s.h[4] = lbf::kH4;
    s.buffered = 0;
    s.total = 0;
    for (int j = 0; j < 64; ++j) s.block[j] = 0;
  }
}

extern "C" int lbf_sha1_update_launch(lbf_sha1_state* d_states, uint64_t n_states, const uint32_t* d_state_of,
                                      const uint8_t* d_base, const uint64_t* d_offsets, const uint32_t* d_sizes,
                                      const uint8_t* d_final, uint64_t n, uint8_t* d_digests,
                                      const uint8_t* d_expected, uint8_t* d_verdicts, void* stream) {
  const char* who = "lbf_sha1_update_launch";
  if (n == 0) return LBF_OK;
  if (!d_states || !d_base || !d_offsets || !d_sizes) return fail(LBF_ERR_INVALID, std::string(who) + ": null input");
  if (n > 0xFFFFFFFFull) return fail(LBF_ERR_INVALID, std::string(who) + ": n exceeds 2^32-1 per launch");
  // a launch with final pieces has something to report; one without needs no output
  if (d_final && !d_digests && !d_verdicts) return fail(LBF_ERR_INVALID, std::string(who) + ": no output");
  if ((d_verdicts != nullptr) != (d_expected != nullptr))
    return fail(LBF_ERR_INVALID, std::string(who) + ": expected and verdicts go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
    return fail(LBF_ERR_INVALID, std::string(who) + ": digest/expected arrays must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_states) & 15u)
    return fail(LBF_ERR_INVALID, std::string(who) + ": the state array must be 16-byte aligned");
  if (n_states > UINT64_MAX / 96) return fail(LBF_ERR_INVALID, std::string(who) + ": n_states too large");
  if (int rc = lbf::tables_fit(who, {{d_states, 96, n_states, "states", false},
                                      {d_state_of, 4, n, "state_of", false},
                                      {d_offsets, 8, n, "offsets", false},
                                      {d_sizes, 4, n, "sizes", false},
                                      {d_final, 1, n, "final", false},
                                      {d_digests, 20, n, "digests", false},
                                      {d_expected, 20, n, "expected", false},
                                      {d_verdicts, 1, n, "verdicts", false}}))
    return rc;
  lbf::UpdateParams p{};
  p.states = reinterpret_cast<uint8_t*>(d_states);
  p.n_states = n_states;
  p.state_of = d_state_of;
  p.base = d_base;
  p.offsets = d_offsets;
  p.sizes = d_sizes;
  p.final_flags = d_final;
  p.n = (uint32_t)n;
  p.digests = d_digests;
  p.expected = d_expected;
  p.verdicts = d_verdicts;
  // 64-thread workgroups while waves are scarce so they spread over every CU (as launch_lane)
  const uint32_t threads = p.n <= 65536u ? 64u : 256u;
  hipLaunchKernelGGL(lbf::sha1_update_kernel, dim3((p.n + threads - 1) / threads), dim3(threads), 0,
                     (hipStream_t)stream, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}
