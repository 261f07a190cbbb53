// b64_update_seq.hip -- the piecewise base64 decode for several pieces of one
// chain per launch: one workgroup per CHAIN, which decodes the chain's pieces
// in the order the chain table gives them (sha1_update_seq.hip has the table)
// and holds the decoder's record in registers from the first piece to the
// last.  lbf_b64_update_seq_launch is three enqueues whatever the piece count:
// this kernel, lbf_sha1_update_seq_launch over the piece table it writes, and
// the length check of final pieces.
//
// Per piece the kernel does what b64_update_fused_kernel does -- line stage,
// flat stage, scan, with lbf_set_b64_lines / lbf_set_b64_flat as the stage mask
// -- from the same stage functions (b64_update_stages.hpp), and writes the same
// piece_off / piece_size / out_sizes and per-stage counts at the piece's index.
// A final piece restarts the record in registers; the record in memory is
// written once, behind the chain's last piece.
//
// Barriers: every one is reached by the whole workgroup.  The chain's piece
// range and each piece's cap are the same in every lane, so a refused piece
// (cap over 1 GiB) is a `continue` taken by all of them; the decode table is
// published by a barrier of its own in front of the loop, whether or not the
// first piece is refused; and one barrier ends each piece, between the scan's
// last reads of LDS and the next piece's first writes.  wave_bad, sums and
// first_eq are written by the stages before they read them, piece by piece.
//
// The route does not depend on lbf_set_b64_fused.  A translation unit of its
// own: the other kernels' ISA stays as recorded.  DESIGN.md §4.9.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "b64_flat.hpp"
#include "b64_update_fused.hpp"
#include "b64_update_lines.hpp"
#include "lbf_internal.hpp"

// The stage functions' lane number, for this translation unit only: the
// hardware's, behind an empty asm at every use.  The stages are full of lane
// predicates (the scan's `lane >= off`, `wave > w`, `threadIdx.x < 3`, ...),
// each a pair of scalar registers.  In the kernels of one piece per workgroup
// the compiler hoists them in front of the stage's own loop; with a loop over
// the chain's pieces around the three stages it hoists all of them in front of
// THAT loop, where they stay live through every stage and push scalar registers
// out into vector lanes (44 of them, and never fewer than 2 however the
// kernel's own values were arranged).  Opaque, each predicate is worked out
// where it is used -- a compare -- and the kernel needs no spill: 97 vector
// registers, 4 waves a SIMD, against 124 and 44 scalars spilled without.
namespace lbf {
namespace b64s {
struct SeqLane {
  uint32_t x;
};
__device__ __forceinline__ SeqLane seq_lane() {
  uint32_t x = threadIdx.x;
  asm volatile("" : "+v"(x));
  return SeqLane{x};
}
}  // namespace b64s
}  // namespace lbf
// b64_device.hpp's helpers (the staging, the scan) read the lane number too: that header is first included from
// the stages header, inside the definition below, and nothing above may include it.
#define threadIdx (::lbf::b64s::seq_lane())
#include "b64_update_stages.hpp"
#undef threadIdx

namespace lbf {

namespace {

struct B64SeqParams {
  uint8_t* b64_states;          // n_states records of 16 bytes, 16-byte aligned
  uint64_t n_states;
  const uint32_t* chain_state;  // state pair of each chain, or null: chain c -> pair c
  const uint32_t* chain_first;  // n_chains + 1 entries
  uint32_t n_chains;
  uint32_t n;
  const uint8_t* text;
  const uint64_t* text_off;
  const uint32_t* text_len;
  const uint8_t* final_flags;   // null => no piece is final
  uint8_t* out;
  const uint64_t* out_off;
  const uint32_t* cap;
  uint32_t* out_sizes;          // written for final pieces only
  uint64_t* piece_off;          // the table lbf_sha1_update_seq_launch reads
  uint32_t* piece_size;
  uint32_t* line_chars;         // null, or n entries (written when the line stage is on)
  uint32_t* flat_chars;         // null, or n entries (written when the flat stage is on)
  uint8_t* verdicts;            // the length check only
  uint32_t stages;              // kB64StageLines | kB64StageFlat
};

using namespace b64s;

// The kernel's parameters where the launch put them (the by-value struct is
// the kernel's only argument, at the start of the kernel argument segment),
// behind an empty asm that hides from the compiler that they are the same every
// time.  The loop below reads what a piece needs through this where it needs
// it -- scalar loads that hit the constant cache -- so that the parameter
// block's nineteen pointers are not loaded at the kernel's entry and held in
// scalar registers across the stages of every piece (12 scalar registers
// spilled, read through `p`).
typedef const B64SeqParams __attribute__((address_space(4))) * KernArgs;
__device__ __forceinline__ KernArgs kernargs() {
  KernArgs k = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// blockIdx.x = chain.
__global__ void __launch_bounds__(kThreads) b64_update_seq_kernel(B64SeqParams p) {
  const uint32_t c = blockIdx.x;
  const uint64_t si = p.chain_state ? (uint64_t)p.chain_state[c] : (uint64_t)c;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written (the whole workgroup leaves)
  uint32_t lo = p.chain_first[c], hi = p.chain_first[c + 1];
  lo = lo < p.n ? lo : p.n;
  hi = hi < p.n ? hi : p.n;
  if (lo >= hi) return;  // no piece: the record is left as it is (the whole workgroup leaves)
  // the tile stages' stage[2][kStage] and the scan's sx[kSx], one after the other
  __shared__ __attribute__((aligned(16))) uint8_t lds[kStageBytes];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t wave_bad[2][kWaves];
  __shared__ uint32_t sums[kWaves];
  __shared__ uint32_t first_eq;
  uint4(*const stage)[kStage] = reinterpret_cast<uint4(*)[kStage]>(lds);

  Rec r = read_rec(p.b64_states + 16 * si);
  bool touched = false;  // a piece moved the record on, or ended the chain
  tab[threadIdx.x] = (uint8_t)value(threadIdx.x);
  __syncthreads();  // the table, whichever piece is the first to use it

  // lo, hi and each piece's cap, final flag and text are the same in every lane.  What is needed only behind a
  // stage (where its count goes, the final flag, the output tables, the record's address) is read there, not
  // carried through the stages: they leave no scalar register free.
  for (uint32_t i = lo; i < hi; ++i) {
    const KernArgs a = kernargs();
    const uint32_t cap = a->cap[i];
    if (cap > kMaxCap) {  // refused: nothing decoded, nothing for the hash, verdict 0
      const bool fin = a->final_flags != nullptr && a->final_flags[i] != 0;
      if (threadIdx.x == 0) {
        a->piece_off[i] = 0;
        a->piece_size[i] = 0;
        if ((a->stages & kB64StageLines) && a->line_chars) a->line_chars[i] = 0;
        if ((a->stages & kB64StageFlat) && a->flat_chars) a->flat_chars[i] = 0;
        if (fin) a->out_sizes[i] = 0;
      }
      if (fin) {  // the hash ends the chain on its empty piece: the pair stays a pair
        r = Rec{0, 0u, 0u, false};
        touched = true;
      }
      continue;  // no LDS was touched: no barrier is owed
    }
    // the piece's share of the chunk starts here (finish_piece's `before`: the chain's position, clipped to the slot)
    const uint32_t before = r.decoded < cap ? (uint32_t)r.decoded : cap;
    const uint8_t* const t = a->text + a->text_off[i];
    const uint32_t len = a->text_len[i];
    const uint64_t slot = a->out_off[i];
    uint8_t* const out = a->out;
    uint32_t taken = 0;  // the same in every lane
    if (a->stages & kB64StageLines) {
      taken = lines_stage(r, Piece{t, len, out, slot, cap}, stage, tab, wave_bad, true);
      const KernArgs k = kernargs();
      if (threadIdx.x == 0 && k->line_chars) k->line_chars[i] = taken;
      __syncthreads();  // the stage's last reads of LDS
    }
    if (kernargs()->stages & kB64StageFlat) {
      const uint32_t flat = flat_stage(r, Piece{t + taken, len - taken, out, slot, cap}, stage, tab, wave_bad);
      taken += flat;
      const KernArgs k = kernargs();
      if (threadIdx.x == 0 && k->flat_chars) k->flat_chars[i] = flat;
      __syncthreads();  // the stage's last reads of LDS
    }
    scan_stage(r, Piece{t + taken, len - taken, out, slot, cap}, lds, tab, sums, &first_eq);
    const KernArgs b = kernargs();
    const bool fin = b->final_flags != nullptr && b->final_flags[i] != 0;
    if (threadIdx.x == 0) {  // finish_piece's table entry and length; the record stays in registers
      const uint32_t after = r.decoded < cap ? (uint32_t)r.decoded : cap;
      b->piece_off[i] = slot + before;
      b->piece_size[i] = after > before ? after - before : 0u;  // decoded never falls; checked all the same
      if (fin) b->out_sizes[i] = r.decoded <= cap ? (uint32_t)r.decoded : cap + 1u;
    }
    if (fin) r = Rec{0, 0u, 0u, false};  // Final() restarts the chain; an unfinished group is dropped
    touched = true;
    __syncthreads();  // the scan's last reads of LDS, before the next piece's first writes
  }
  if (touched && threadIdx.x == 0) {
    const KernArgs e = kernargs();
    uint32_t ch = blockIdx.x;
    asm volatile("" : "+s"(ch));  // or its offset into the table is carried from the top
    const uint64_t s = e->chain_state ? (uint64_t)e->chain_state[ch] : (uint64_t)ch;  // si, read again
    if (s < e->n_states) *reinterpret_cast<uint4*>(e->b64_states + 16 * s) = rec_words(r);
  }
}

// A final piece's verdict holds only when its text decoded to the chunk's size
// (ChunkMethods.cpp:156), as b64_length_kernel checks it per piece; one lane
// per chain here, so pieces that no chain names are left alone.
__global__ void __launch_bounds__(256) b64_length_seq_kernel(B64SeqParams p) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= p.n_chains) return;
  const uint64_t si = p.chain_state ? (uint64_t)p.chain_state[c] : (uint64_t)c;
  if (si >= p.n_states) return;
  uint32_t lo = p.chain_first[c], hi = p.chain_first[c + 1];
  lo = lo < p.n ? lo : p.n;
  hi = hi < p.n ? hi : p.n;
  for (uint32_t i = lo; i < hi; ++i) {
    if (!p.final_flags[i]) continue;
    const uint32_t cap = p.cap[i];
    if (cap > kMaxCap || p.out_sizes[i] != cap) p.verdicts[i] = 0;
  }
}

}  // namespace

}  // namespace lbf

using lbf::fail;

extern "C" int lbf_b64_update_seq_launch(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                         const uint32_t* d_chain_state, const uint32_t* d_chain_first,
                                         uint64_t n_chains, const char* d_text, const uint64_t* d_text_offsets,
                                         const uint32_t* d_text_lens, const uint8_t* d_final, uint64_t n,
                                         uint8_t* d_out, const uint64_t* d_out_offsets, const uint32_t* d_caps,
                                         uint32_t* d_out_sizes, uint8_t* d_digests, const uint8_t* d_expected,
                                         uint8_t* d_verdicts, uint64_t* d_piece_offsets, uint32_t* d_piece_sizes,
                                         void* stream) {
  return lbf::b64_update_seq_launch_counted(d_b64_states, d_sha_states, n_states, d_chain_state, d_chain_first,
                                            n_chains, d_text, d_text_offsets, d_text_lens, d_final, n, d_out,
                                            d_out_offsets, d_caps, d_out_sizes, d_digests, d_expected, d_verdicts,
                                            d_piece_offsets, d_piece_sizes, nullptr, nullptr, stream);
}

int lbf::b64_update_seq_launch_counted(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                       const uint32_t* d_chain_state, const uint32_t* d_chain_first, uint64_t n_chains,
                                       const char* d_text, const uint64_t* d_text_offsets, const uint32_t* d_text_lens,
                                       const uint8_t* d_final, uint64_t n, uint8_t* d_out,
                                       const uint64_t* d_out_offsets, const uint32_t* d_caps, uint32_t* d_out_sizes,
                                       uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                                       uint64_t* d_piece_offsets, uint32_t* d_piece_sizes, uint32_t* d_line_chars,
                                       uint32_t* d_flat_chars, void* stream) {
  const std::string who = "lbf_b64_update_seq_launch";
  if (n == 0 || n_chains == 0) return LBF_OK;
  if (!d_b64_states || !d_sha_states || !d_chain_first || !d_text || !d_text_offsets || !d_text_lens || !d_out ||
      !d_out_offsets || !d_caps || !d_out_sizes || !d_piece_offsets || !d_piece_sizes)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  if (n_chains > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n_chains exceeds 2^31-1 per launch");
  // what lbf_sha1_update_seq_launch would refuse is refused here, before the decode is enqueued
  if (d_final && !d_digests && !d_verdicts) return fail(LBF_ERR_INVALID, who + ": no output");
  if ((d_verdicts != nullptr) != (d_expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digest/expected arrays must be 4-byte aligned");
  if ((reinterpret_cast<uintptr_t>(d_b64_states) & 15u) || (reinterpret_cast<uintptr_t>(d_sha_states) & 15u))
    return fail(LBF_ERR_INVALID, who + ": the state arrays must be 16-byte aligned");
  const std::initializer_list<lbf::DevTable> tables = {
      {d_b64_states, 16, n_states, "b64_states", false},
      {d_sha_states, 96, n_states, "sha_states", false},
      {d_chain_state, 4, n_chains, "chain_state", true},
      {d_chain_first, 4, n_chains + 1, "chain_first", true},
      {d_text_offsets, 8, n, "text_offsets", true},
      {d_text_lens, 4, n, "text_lens", true},
      {d_final, 1, n, "final", false},
      {d_out_offsets, 8, n, "out_offsets", true},
      {d_caps, 4, n, "caps", true},
      {d_out_sizes, 4, n, "out_sizes", true},
      {d_digests, 20, n, "digests", false},
      {d_expected, 20, n, "expected", false},
      {d_verdicts, 1, n, "verdicts", false},
      {d_piece_offsets, 8, n, "piece_offsets", true},
      {d_piece_sizes, 4, n, "piece_sizes", true},
      {d_line_chars, 4, n, "line_chars", false},
      {d_flat_chars, 4, n, "flat_chars", false}};
  if (int rc = lbf::tables_aligned(who, tables)) return rc;
  if (n_states > UINT64_MAX / 96) return fail(LBF_ERR_INVALID, who + ": n_states too large");
  if (int rc = lbf::tables_fit(who, tables)) return rc;
  lbf::B64SeqParams p{};
  p.b64_states = reinterpret_cast<uint8_t*>(d_b64_states);
  p.n_states = n_states;
  p.chain_state = d_chain_state;
  p.chain_first = d_chain_first;
  p.n_chains = (uint32_t)n_chains;
  p.n = (uint32_t)n;
  p.text = reinterpret_cast<const uint8_t*>(d_text);
  p.text_off = d_text_offsets;
  p.text_len = d_text_lens;
  p.final_flags = d_final;
  p.out = d_out;
  p.out_off = d_out_offsets;
  p.cap = d_caps;
  p.out_sizes = d_out_sizes;
  p.piece_off = d_piece_offsets;
  p.piece_size = d_piece_sizes;
  p.line_chars = d_line_chars;
  p.flat_chars = d_flat_chars;
  p.verdicts = d_verdicts;
  p.stages = (lbf::b64_lines_enabled() ? lbf::kB64StageLines : 0u) | (lbf::b64_flat_enabled() ? lbf::kB64StageFlat : 0u);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lbf::b64_update_seq_kernel, dim3(p.n_chains), dim3(lbf::b64s::kThreads), 0, st, p);
  LBF_HIP_TRY(hipGetLastError());
  if (int rc = lbf_sha1_update_seq_launch(d_sha_states, n_states, d_chain_state, d_chain_first, n_chains, d_out,
                                          d_piece_offsets, d_piece_sizes, d_final, n, d_digests, d_expected,
                                          d_verdicts, st))
    return rc;
  if (d_final && d_verdicts) {
    hipLaunchKernelGGL(lbf::b64_length_seq_kernel, dim3((p.n_chains + 255u) / 256u), dim3(256), 0, st, p);
    LBF_HIP_TRY(hipGetLastError());
  }
  return LBF_OK;
}
