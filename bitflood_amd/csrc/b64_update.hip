// b64_update.hip -- resumable base64 decode on the GPU, chained on the device
// to the resumable SHA-1: one piece of a chunk's text per workgroup, continued
// from a caller-owned 16-byte state (lbf_b64_state, lbf_hash.h).
//
// A SendChunk payload arrives as text, in pieces (ChunkMethods.cpp:137-167).
// The general decode of kern_b64.hpp needs a chunk's whole text; here the
// decoder of xmlrpc++ 0.7 (base64.h:215-330) is stopped between pieces: the
// sextets of an unfinished group are carried in the record, the first '=' ends
// the data for good, and on the final piece an unfinished group is dropped.
// The decoded bytes land in the chunk's slot at their position in the chunk,
// a piece table says where each piece's new bytes lie, and
// lbf_sha1_update_launch absorbs exactly those: the verdict waits only for the
// last piece's share of the chunk.
//
// The kernel here treats a piece as arbitrary text.  The part of a piece that
// continues the encoder's layout is taken first by b64_update_lines.hip's
// kernel (unless lbf_set_b64_lines switched it off), which moves the record on
// and hands over, through the piece table's two arrays, where the chain stood
// and how many characters it took; unbroken text in what that left is taken
// next by b64_flat.hip's kernel (lbf_set_b64_flat), which hands over the same
// two numbers; this kernel decodes what is left.  With lbf_set_b64_fused on,
// one kernel (b64_update_fused.hip) runs the three stages of a piece in one
// launch instead, and the two switches are its stage mask.  All four kernels
// are built from the stage functions of b64_update_stages.hpp.
//
// A translation unit of its own, like sha1_update.hip: the shipped kernels'
// ISA stays as recorded (tests/test_isa.py).  DESIGN.md §4.7.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>

#include <atomic>

#include "b64_flat.hpp"
#include "b64_update_fused.hpp"
#include "b64_update_lines.hpp"
#include "b64_update_stages.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

struct B64UpdateParams {
  uint8_t* b64_states;          // n_states records of 16 bytes, 16-byte aligned
  uint64_t n_states;
  const uint32_t* state_of;     // chain of each piece, or null: piece i -> chain i
  const uint8_t* text;
  const uint64_t* text_off;
  const uint32_t* text_len;
  const uint8_t* final_flags;   // null => no piece is final
  uint8_t* out;
  const uint64_t* out_off;      // the chunk's slot ...
  const uint32_t* cap;          // ... and its size
  uint32_t* out_sizes;          // written for final pieces only
  uint64_t* piece_off;          // the table lbf_sha1_update_launch reads
  uint32_t* piece_size;
  uint8_t* verdicts;            // the last kernel only
  // the line path ran in front (b64_update_lines.hip): piece_off[i] holds the chain's byte count before the call
  // and piece_size[i] the characters of the piece already decoded; both are overwritten with their final values
  uint32_t lines;
};

using namespace b64s;

// blockIdx.x = piece.  The trips are scan_stage's (b64_update_stages.hpp), which
// the fused kernel (b64_update_fused.hip) runs too.
__global__ void __launch_bounds__(kThreads) b64_update_kernel(B64UpdateParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written (the whole workgroup leaves)
  const uint32_t cap = p.cap[i];
  const bool fin = p.final_flags != nullptr && p.final_flags[i] != 0;
  if (cap > kMaxCap) {  // refused: nothing decoded, nothing for the hash, verdict 0 (b64_length_kernel)
    if (threadIdx.x == 0) {
      p.piece_off[i] = 0;
      p.piece_size[i] = 0;
      if (fin) {
        // the update kernel ends the chain on its empty piece and restarts the SHA record: the pair stays a pair
        p.out_sizes[i] = 0;
        *reinterpret_cast<uint4*>(p.b64_states + 16 * si) = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) uint8_t sx[kSx];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t sums[kWaves];
  __shared__ uint32_t first_eq;

  uint8_t* const rec = p.b64_states + 16 * si;
  Rec r = read_rec(rec);
  uint64_t start = r.decoded;
  uint32_t taken = 0;
  if (p.lines) {  // the record has moved on by what the line path took: the piece's share starts where it started
    start = p.piece_off[i];
    taken = p.piece_size[i];
  }
  tab[threadIdx.x] = (uint8_t)value(threadIdx.x);
  const uint32_t piece_len = p.text_len[i];
  if (taken > piece_len) taken = piece_len;  // never: the line path takes a prefix
  const uint64_t slot = p.out_off[i];
  const Piece pc{p.text + p.text_off[i] + taken, piece_len - taken, p.out, slot, cap};
  scan_stage(r, pc, sx, tab, sums, &first_eq);
  if (threadIdx.x == 0)
    finish_piece(r, start, slot, cap, fin, rec, p.piece_off + i, p.piece_size + i, p.out_sizes + i);
}

// A final piece's verdict holds only when its text decoded to the chunk's size
// (ChunkMethods.cpp:156): out_sizes[i] is the decoded length, or cap + 1.
__global__ void __launch_bounds__(256) b64_length_kernel(B64UpdateParams p, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !p.final_flags[i]) return;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;
  const uint32_t cap = p.cap[i];
  if (cap > kMaxCap || p.out_sizes[i] != cap) p.verdicts[i] = 0;
}

}  // namespace

}  // namespace lbf

using lbf::fail;

extern "C" void lbf_b64_state_init(lbf_b64_state* states, uint64_t n) {
  if (!states) return;
  for (uint64_t k = 0; k < n; ++k) {
    lbf_b64_state& s = states[k];
    s.decoded = 0;
    s.carry = 0;
    s.ncarry = 0;
    s.ended = 0;
    s.zero = 0;
  }
}

// The line path's switch: LBF_B64_LINES at first use (default on), then lbf_set_b64_lines.
static std::atomic<int> g_b64_lines{-1};

bool lbf::b64_lines_enabled() {
  int v = g_b64_lines.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("LBF_B64_LINES");
    const int from_env = lbf::kB64LinesDefault ? !(e && e[0] == '0' && e[1] == 0) : (e && e[0] == '1' && e[1] == 0);
    g_b64_lines.compare_exchange_strong(v, from_env, std::memory_order_relaxed);  // a setter that got in first wins
    v = g_b64_lines.load(std::memory_order_relaxed);
  }
  return v != 0;
}

extern "C" int lbf_set_b64_lines(int on) {
  const int before = lbf::b64_lines_enabled() ? 1 : 0;
  g_b64_lines.store(on ? 1 : 0, std::memory_order_relaxed);
  return before;
}

extern "C" int lbf_b64_update_launch(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                     const uint32_t* d_state_of, const char* d_text, const uint64_t* d_text_offsets,
                                     const uint32_t* d_text_lens, const uint8_t* d_final, uint64_t n, uint8_t* d_out,
                                     const uint64_t* d_out_offsets, const uint32_t* d_caps, uint32_t* d_out_sizes,
                                     uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                                     uint64_t* d_piece_offsets, uint32_t* d_piece_sizes, void* stream) {
  return lbf::b64_update_launch_counted(d_b64_states, d_sha_states, n_states, d_state_of, d_text, d_text_offsets,
                                        d_text_lens, d_final, n, d_out, d_out_offsets, d_caps, d_out_sizes, d_digests,
                                        d_expected, d_verdicts, d_piece_offsets, d_piece_sizes, nullptr, nullptr,
                                        stream);
}

int lbf::b64_update_launch_counted(lbf_b64_state* d_b64_states, lbf_sha1_state* d_sha_states, uint64_t n_states,
                                   const uint32_t* d_state_of, const char* d_text, const uint64_t* d_text_offsets,
                                   const uint32_t* d_text_lens, const uint8_t* d_final, uint64_t n, uint8_t* d_out,
                                   const uint64_t* d_out_offsets, const uint32_t* d_caps, uint32_t* d_out_sizes,
                                   uint8_t* d_digests, const uint8_t* d_expected, uint8_t* d_verdicts,
                                   uint64_t* d_piece_offsets, uint32_t* d_piece_sizes, uint32_t* d_line_chars,
                                   uint32_t* d_flat_chars, void* stream) {
  const std::string who = "lbf_b64_update_launch";
  if (n == 0) return LBF_OK;
  if (!d_b64_states || !d_sha_states || !d_text || !d_text_offsets || !d_text_lens || !d_out || !d_out_offsets ||
      !d_caps || !d_out_sizes || !d_piece_offsets || !d_piece_sizes)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  // what lbf_sha1_update_launch would refuse is refused here, before the decode is enqueued
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
      {d_state_of, 4, n, "state_of", true},
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
  lbf::B64UpdateParams p{};
  p.b64_states = reinterpret_cast<uint8_t*>(d_b64_states);
  p.n_states = n_states;
  p.state_of = d_state_of;
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
  p.verdicts = d_verdicts;
  hipStream_t st = (hipStream_t)stream;
  if (lbf::b64_fused_enabled()) {  // the three decode kernels in one launch; the two switches are its stage mask
    lbf::B64FusedParams f{};
    f.b64_states = p.b64_states;
    f.n_states = n_states;
    f.state_of = d_state_of;
    f.text = p.text;
    f.text_off = d_text_offsets;
    f.text_len = d_text_lens;
    f.final_flags = d_final;
    f.out = d_out;
    f.out_off = d_out_offsets;
    f.cap = d_caps;
    f.out_sizes = d_out_sizes;
    f.piece_off = d_piece_offsets;
    f.piece_size = d_piece_sizes;
    f.line_chars = d_line_chars;
    f.flat_chars = d_flat_chars;
    f.stages = (lbf::b64_lines_enabled() ? lbf::kB64StageLines : 0u) |
               (lbf::b64_flat_enabled() ? lbf::kB64StageFlat : 0u);
    if (int rc = lbf::launch_b64_update_fused(f, (uint32_t)n, st)) return rc;
  } else {
    if (lbf::b64_lines_enabled()) {  // the text that continues the encoder's layout, in front of the general rule
      lbf::B64LinesParams lp{};
      lp.b64_states = p.b64_states;
      lp.n_states = n_states;
      lp.state_of = d_state_of;
      lp.text = p.text;
      lp.text_off = d_text_offsets;
      lp.text_len = d_text_lens;
      lp.out = d_out;
      lp.out_off = d_out_offsets;
      lp.cap = d_caps;
      lp.before = d_piece_offsets;
      lp.taken = d_piece_sizes;
      lp.line_chars = d_line_chars;
      if (int rc = lbf::launch_b64_update_lines(lp, (uint32_t)n, st)) return rc;
      p.lines = 1;
    }
    if (lbf::b64_flat_enabled()) {  // unbroken text in what is left: the same hand-over
      lbf::B64FlatParams fp{};
      fp.b64_states = p.b64_states;
      fp.n_states = n_states;
      fp.state_of = d_state_of;
      fp.text = p.text;
      fp.text_off = d_text_offsets;
      fp.text_len = d_text_lens;
      fp.out = d_out;
      fp.out_off = d_out_offsets;
      fp.cap = d_caps;
      fp.before = d_piece_offsets;
      fp.taken = d_piece_sizes;
      fp.flat_chars = d_flat_chars;
      fp.after_lines = p.lines;
      if (int rc = lbf::launch_b64_update_flat(fp, (uint32_t)n, st)) return rc;
      p.lines = 1;
    }
    hipLaunchKernelGGL(lbf::b64_update_kernel, dim3((uint32_t)n), dim3(lbf::kThreads), 0, st, p);
    LBF_HIP_TRY(hipGetLastError());
  }
  if (int rc = lbf_sha1_update_launch(d_sha_states, n_states, d_state_of, d_out, d_piece_offsets, d_piece_sizes,
                                      d_final, n, d_digests, d_expected, d_verdicts, st))
    return rc;
  if (d_final && d_verdicts) {
    hipLaunchKernelGGL(lbf::b64_length_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, p, (uint32_t)n);
    LBF_HIP_TRY(hipGetLastError());
  }
  return LBF_OK;
}
