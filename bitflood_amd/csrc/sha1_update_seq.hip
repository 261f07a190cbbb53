// sha1_update_seq.hip -- resumable SHA-1 on the GPU, several pieces of one
// chain per launch: one lane per CHAIN, which absorbs the chain's pieces in the
// order the chain table gives them and holds the record's header (h, buffered,
// total) in registers from the first piece to the last.
//
// sha1_update.hip maps a lane to a piece, reads the record at the start and
// writes it at the end, so two pieces of one chain in one launch have no
// defined order there.  A receiver that drains its sockets on a deadline holds
// several frames of the same chunk; here they go in one launch.  The chain
// table is CSR: chain c continues state chain_state[c] (state c without the
// array) and its pieces are the piece indices [chain_first[c], chain_first[c +
// 1]), absorbed in index order.  Outputs stay indexed by piece.  A final piece
// that is not its chain's last ends the chunk, writes its outputs, and the
// pieces behind it begin a new chunk from the initial value -- what successive
// launches of sha1_update.hip give.
//
// Only the 64-byte block goes through the record in memory, topped up
// byte-wise as in sha1_update.hip (a register array indexed by `buffered` would
// live in scratch); the 32 header bytes are read once and written once.
//
// The block loops are sha1_device.hpp's, the record's layout, finish64 and a
// final piece's outputs sha1_resume.hpp's, as in sha1_update.hip.  DESIGN.md §4.9.
#include <hip/hip_runtime.h>

#include "lbf_internal.hpp"
#include "sha1_resume.hpp"

namespace lbf {

namespace {

struct UpdateSeqParams {
  uint8_t* states;              // n_states records of 96 bytes, 16-byte aligned
  uint64_t n_states;
  const uint32_t* chain_state;  // state of each chain, or null: chain c -> state c
  const uint32_t* chain_first;  // n_chains + 1 entries: chain c's pieces are [first[c], first[c + 1])
  uint32_t n_chains;
  const uint8_t* base;
  const uint64_t* offsets;
  const uint32_t* sizes;
  const uint8_t* final_flags;   // null => no piece is final
  uint32_t n;
  uint8_t* digests;             // n*20 or null; written for final pieces only
  const uint8_t* expected;      // n*20 or null
  uint8_t* verdicts;            // n or null; written for final pieces only
};

__global__ void __launch_bounds__(256) sha1_update_seq_kernel(UpdateSeqParams p) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= p.n_chains) return;
  const uint64_t si = p.chain_state ? (uint64_t)p.chain_state[c] : (uint64_t)c;
  if (si >= p.n_states) return;  // names no state: nothing is read or written for the chain
  // both ends clamped to n; an inverted range is empty
  uint32_t lo = p.chain_first[c], hi = p.chain_first[c + 1];
  lo = lo < p.n ? lo : p.n;
  hi = hi < p.n ? hi : p.n;
  if (lo >= hi) return;  // no piece: the record is left as it is
  uint8_t* const rec = p.states + kStateBytes * si;
  uint8_t* const blk = rec + kBlockAt;
  uint4* const out = reinterpret_cast<uint4*>(rec);

  const uint4 h03 = out[0];  // h[0..3]
  const uint4 h4 = out[1];   // h[4], buffered, total
  Digest s;
  s.h[0] = h03.x; s.h[1] = h03.y; s.h[2] = h03.z; s.h[3] = h03.w; s.h[4] = h4.x;
  // & 63: whatever a forged record says, every byte index below stays inside
  // the record's own 64-byte block
  uint32_t buf = h4.y & 63u;
  uint64_t total = (uint64_t)h4.z | ((uint64_t)h4.w << 32);

  for (uint32_t i = lo; i < hi; ++i) {
    const uint8_t* src = p.base + p.offsets[i];
    uint32_t size = p.sizes[i];
    const bool fin = p.final_flags != nullptr && p.final_flags[i] != 0;
    total += size;

    if (buf) {
      // top the unfinished block up in the record itself and read it back whole
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
    if (nblk) {  // the loop is chosen per piece, by where its full blocks start
      if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        hash_blocks_aligned(s, src, nblk);
      } else {
        hash_blocks_unaligned(s, src, nblk);
      }
      src += 64ull * nblk;
    }
    const uint32_t rem = size & 63u;  // non-zero only with buf == 0
    for (uint32_t k = 0; k < rem; ++k) blk[(buf + k) & 63u] = src[k];
    buf = (buf + rem) & 63u;
    if (!fin) continue;

    uint32_t w[16];
    record_block(w, blk);
    finish64(s, w, buf, total);
    uint32_t be[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) be[k] = bswap(s.h[k]);  // digest bytes in big-endian order
    write_final(p, i, be);
    // Final() restarts the object (iterhash.h:120): the registers and the block
    // are as lbf_sha1_state_init leaves them, and the pieces that follow begin
    // a new chunk
    s.h[0] = kH0; s.h[1] = kH1; s.h[2] = kH2; s.h[3] = kH3; s.h[4] = kH4;
    buf = 0;
    total = 0;
#pragma unroll
    for (int k = 2; k < 6; ++k) out[k] = make_uint4(0u, 0u, 0u, 0u);
  }

  out[0] = make_uint4(s.h[0], s.h[1], s.h[2], s.h[3]);
  out[1] = make_uint4(s.h[4], buf, (uint32_t)total, (uint32_t)(total >> 32));
}

}  // namespace

}  // namespace lbf

using lbf::fail;

extern "C" int lbf_sha1_update_seq_launch(lbf_sha1_state* d_states, uint64_t n_states, const uint32_t* d_chain_state,
                                          const uint32_t* d_chain_first, uint64_t n_chains, const uint8_t* d_base,
                                          const uint64_t* d_offsets, const uint32_t* d_sizes, const uint8_t* d_final,
                                          uint64_t n, uint8_t* d_digests, const uint8_t* d_expected,
                                          uint8_t* d_verdicts, void* stream) {
  const std::string who = "lbf_sha1_update_seq_launch";
  if (n == 0 || n_chains == 0) return LBF_OK;
  if (!d_states || !d_chain_first || !d_base || !d_offsets || !d_sizes)
    return fail(LBF_ERR_INVALID, who + ": null input");
  if (n > 0xFFFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^32-1 per launch");
  if (n_chains > 0xFFFFFFFEull) return fail(LBF_ERR_INVALID, who + ": n_chains exceeds 2^32-2 per launch");
  // a launch with final pieces has something to report; one without needs no output
  if (d_final && !d_digests && !d_verdicts) return fail(LBF_ERR_INVALID, who + ": no output");
  if ((d_verdicts != nullptr) != (d_expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digest/expected arrays must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(d_states) & 15u)
    return fail(LBF_ERR_INVALID, who + ": the state array must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_chain_state) & 3u) || (reinterpret_cast<uintptr_t>(d_chain_first) & 3u))
    return fail(LBF_ERR_INVALID, who + ": the chain table must be 4-byte aligned");
  if (n_states > UINT64_MAX / 96) return fail(LBF_ERR_INVALID, who + ": n_states too large");
  if (int rc = lbf::tables_fit(who, {{d_states, 96, n_states, "states", false},
                                      {d_chain_state, 4, n_chains, "chain_state", false},
                                      {d_chain_first, 4, n_chains + 1, "chain_first", false},
                                      {d_offsets, 8, n, "offsets", false},
                                      {d_sizes, 4, n, "sizes", false},
                                      {d_final, 1, n, "final", false},
                                      {d_digests, 20, n, "digests", false},
                                      {d_expected, 20, n, "expected", false},
                                      {d_verdicts, 1, n, "verdicts", false}}))
    return rc;
  lbf::UpdateSeqParams p{};
  p.states = reinterpret_cast<uint8_t*>(d_states);
  p.n_states = n_states;
  p.chain_state = d_chain_state;
  p.chain_first = d_chain_first;
  p.n_chains = (uint32_t)n_chains;
  p.base = d_base;
  p.offsets = d_offsets;
  p.sizes = d_sizes;
  p.final_flags = d_final;
  p.n = (uint32_t)n;
  p.digests = d_digests;
  p.expected = d_expected;
  p.verdicts = d_verdicts;
  // 64-thread workgroups while waves are scarce so they spread over every CU (as lbf_sha1_update_launch)
  const uint32_t threads = p.n_chains <= 65536u ? 64u : 256u;
  hipLaunchKernelGGL(lbf::sha1_update_seq_kernel, dim3((p.n_chains + threads - 1) / threads), dim3(threads), 0,
                     (hipStream_t)stream, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}
