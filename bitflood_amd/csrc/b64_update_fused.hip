// b64_update_fused.hip -- the fused route of the piecewise base64 decode: one
// launch, one workgroup per piece, that does what b64_update_lines_kernel,
// b64_update_flat_kernel and b64_update_kernel do in sequence (b64_update.hip
// has the route, lbf_set_b64_fused switches it).
//
// The three kernels have one shape -- a workgroup of 256 lanes per piece that
// reads the chain's record and takes a prefix of what the one before left --
// and between them they pass the record through global memory and two numbers
// through the piece table's arrays.  Here the record is read once and stays in
// registers, what a stage took is a workgroup-uniform value, and the piece
// table, a final piece's length and the record are written once, behind the
// scan.  The stages are the same device functions the three kernels are built
// from (b64_update_stages.hpp), so each takes, to the character, what it takes
// on the unfused route; which of them takes which characters is decided here,
// per piece, by the text itself.  lbf_set_b64_lines and lbf_set_b64_flat arrive
// as a mask of the stages to run in front of the scan.
//
// LDS: the tile stages' two text buffers (10,688 bytes) and the scan's sextets
// (4,112 bytes) are never live together and share one allocation; the decode
// table is loaded once.  A barrier stands between one stage's last read of LDS
// and the next stage's first write, and every barrier is reached by the whole
// workgroup: the only early exits (a piece that names no chain, a chunk over
// 1 GiB) are taken by every lane before the first barrier.  The one cheap look
// ahead: the line stage tests the first separator place between two of the
// piece's groups before it stages a tile, so unbroken text passes to the flat
// stage at the cost of one byte read, not of a tile decoded and dropped.
//
// A translation unit of its own: the other kernels' ISA stays as recorded.
// DESIGN.md §4.7.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>

#include <atomic>

#include "b64_update_fused.hpp"
#include "b64_update_stages.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

using namespace b64s;

// blockIdx.x = piece.  Eight waves a SIMD, as the three stage kernels: left to
// itself the compiler keeps 105 scalar registers live across the stages, one
// allocation granule past what eight waves leave each; told the bound it parks
// 32 of them in lanes of one vector register (60 in all, no scratch).
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8)))
b64_update_fused_kernel(B64FusedParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written (the whole workgroup leaves)
  const uint32_t cap = p.cap[i];
  const bool fin = p.final_flags != nullptr && p.final_flags[i] != 0;
  uint8_t* const rec = p.b64_states + 16 * si;
  if (cap > kMaxCap) {  // refused: nothing decoded, nothing for the hash, verdict 0 (the whole workgroup leaves)
    if (threadIdx.x == 0) {
      p.piece_off[i] = 0;
      p.piece_size[i] = 0;
      if ((p.stages & kB64StageLines) && p.line_chars) p.line_chars[i] = 0;
      if ((p.stages & kB64StageFlat) && p.flat_chars) p.flat_chars[i] = 0;
      if (fin) {
        // the update kernel ends the chain on its empty piece and restarts the SHA record: the pair stays a pair
        p.out_sizes[i] = 0;
        *reinterpret_cast<uint4*>(rec) = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    return;
  }
  // the tile stages' stage[2][kStage] and the scan's sx[kSx], one after the other
  __shared__ __attribute__((aligned(16))) uint8_t lds[kStageBytes];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t wave_bad[2][kWaves];
  __shared__ uint32_t sums[kWaves];
  __shared__ uint32_t first_eq;
  uint4(*const stage)[kStage] = reinterpret_cast<uint4(*)[kStage]>(lds);

  Rec r = read_rec(rec);
  const uint64_t start = r.decoded;  // the piece's share of the chunk starts here
  tab[threadIdx.x] = (uint8_t)value(threadIdx.x);  // published by the first barrier any stage reaches
  const uint8_t* const t = p.text + p.text_off[i];
  const uint32_t len = p.text_len[i];
  const uint64_t slot = p.out_off[i];
  uint32_t taken = 0, line = 0, flat = 0;  // each the same in every lane
  if (p.stages & kB64StageLines) {
    line = lines_stage(r, Piece{t, len, p.out, slot, cap}, stage, tab, wave_bad, true);
    taken = line;
    __syncthreads();  // the stage's last reads of LDS
  }
  if (p.stages & kB64StageFlat) {
    flat = flat_stage(r, Piece{t + taken, len - taken, p.out, slot, cap}, stage, tab, wave_bad);
    taken += flat;
    __syncthreads();  // the stage's last reads of LDS
  }
  scan_stage(r, Piece{t + taken, len - taken, p.out, slot, cap}, lds, tab, sums, &first_eq);
  if (threadIdx.x == 0) {
    finish_piece(r, start, slot, cap, fin, rec, p.piece_off + i, p.piece_size + i, p.out_sizes + i);
    if ((p.stages & kB64StageLines) && p.line_chars) p.line_chars[i] = line;
    if ((p.stages & kB64StageFlat) && p.flat_chars) p.flat_chars[i] = flat;
  }
}

}  // namespace

int launch_b64_update_fused(const B64FusedParams& p, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(b64_update_fused_kernel, dim3(n), dim3(kThreads), 0, stream, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace lbf

// The fused route's switch: LBF_B64_FUSED at first use, then lbf_set_b64_fused.
static std::atomic<int> g_b64_fused{-1};

bool lbf::b64_fused_enabled() {
  int v = g_b64_fused.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("LBF_B64_FUSED");
    const int from_env = lbf::kB64FusedDefault ? !(e && e[0] == '0' && e[1] == 0) : (e && e[0] == '1' && e[1] == 0);
    g_b64_fused.compare_exchange_strong(v, from_env, std::memory_order_relaxed);  // a setter that got in first wins
    v = g_b64_fused.load(std::memory_order_relaxed);
  }
  return v != 0;
}

extern "C" int lbf_set_b64_fused(int on) {
  const int before = lbf::b64_fused_enabled() ? 1 : 0;
  g_b64_fused.store(on ? 1 : 0, std::memory_order_relaxed);
  return before;
}
