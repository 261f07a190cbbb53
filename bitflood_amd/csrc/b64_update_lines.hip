// b64_update_lines.hip -- the line path of the piecewise base64 decode: the
// part of a piece that continues xmlrpc++'s layout, decoded through tiles of
// whole lines in front of b64_update_kernel (b64_update.hip), which takes the
// rest by the general rule.
//
// Nearly every piece a receiver gets is a cut-out of what the encoder wrote:
// groups of four alphabet characters, one separator after every 18th group.
// The record says where in that layout the piece starts: S = 4 * decoded / 3 +
// ncarry sextets have been taken, so the next character's column is S mod 72
// and every later character's place is known without a scan.  The kernel
// takes the longest prefix it can show to follow the layout, a tile at a time,
// and hands the rest on:
//   - at column 0 one leading character outside the alphabet (and not '=') is
//     the separator -- the record cannot say whether the previous piece held
//     it, and the general rule skips it either way;
//   - a carried group is completed from the next 4 - ncarry characters;
//   - whole groups follow, a separator between a line's 18th group and the
//     next line's first.  The prefix ends behind a group, so nothing is
//     carried, and before a group that holds '='.
// For such a prefix the general rule (skip what is outside the alphabet, take
// the rest four at a time) gives the same bytes: tests/wire_line_model.py.
//
// Tiles are kern_b64.hpp's decode tiles (72 lines: 5,256 characters -> 3,888
// bytes = 243 blocks of 16) laid over the CHUNK, not the piece: block u of
// tile k holds chunk bytes [3888k + 16u, +16).  A piece starts at any byte and
// any column, so the first and last tile of a piece are partial, and a block
// that is not wholly the piece's is written by bytes.  A tile is validated
// before it is stored: every lane decodes its block, the workgroup ORs the
// lanes' flags across one barrier (the same barrier that publishes the next
// tile's text), and a tile that breaks the layout writes nothing and ends the
// prefix at its start.  The kernel never finalises a chain: out_sizes, the
// final piece's dropped carry and the record's reset stay with
// b64_update_kernel.  DESIGN.md §4.7.
//
// A translation unit of its own: the other kernels' ISA stays as recorded.
// The stage itself is lines_stage (b64_update_stages.hpp), which the fused
// kernel (b64_update_fused.hip) runs too; the kernel here reads the record,
// runs the stage and hands over through global memory.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "b64_update_lines.hpp"
#include "b64_update_stages.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

using namespace b64s;

// blockIdx.x = piece.
__global__ void __launch_bounds__(kThreads) b64_update_lines_kernel(B64LinesParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written, the hand-off included
  __shared__ uint4 stage[2][kStage];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t wave_bad[2][kWaves];

  uint8_t* const rec = p.b64_states + 16 * si;
  Rec r = read_rec(rec);
  const uint64_t decoded = r.decoded;
  const uint32_t cap = p.cap[i], len = p.text_len[i];
  uint32_t taken = 0;
  // a chunk or a record the batch call would refuse, or no text: the piece is b64_update_kernel's whole (the whole
  // workgroup: every value is the same in every lane)
  if (cap <= kMaxCap && !nothing_to_take(r, len)) {
    tab[threadIdx.x] = (uint8_t)value(threadIdx.x);
    const Piece pc{p.text + p.text_off[i], len, p.out, p.out_off[i], cap};
    taken = lines_stage(r, pc, stage, tab, wave_bad, false);
  }
  if (threadIdx.x == 0) {
    if (r.decoded != decoded) *reinterpret_cast<uint4*>(rec) = rec_words(r);  // behind a group: nothing is carried
    p.before[i] = decoded;
    p.taken[i] = taken;
    if (p.line_chars) p.line_chars[i] = taken;
  }
}

}  // namespace

int launch_b64_update_lines(const B64LinesParams& p, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(b64_update_lines_kernel, dim3(n), dim3(kThreads), 0, stream, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace lbf
