// b64_verify_launch.hip -- lbf_b64_verify_launch: chunk text resident in
// device memory decoded and verified one-shot, asynchronous on the caller's
// stream, with no host in the middle.
//
// lbf_b64_verify_batch (wire_batch.cpp) needs its host for three things: it
// reorders the chunks by layout so each tile kernel gets a contiguous range, it
// takes the longest text and the largest cap to size the grids, and it lays out
// the sextet scratch of the two-pass general decode with a prefix sum.  Here
// the caller gives the two bounds, and the rest moves to the device:
//
//   hipMemsetAsync             d_work = over[n] | redo[n], zeroed.
//   b64_decode_routed_kernel   grid = (groups of 4 tiles, chunks), at most
//       65,535 chunks per launch.  Every workgroup routes its chunk from the
//       chunk's own lengths, before any barrier and the same in every lane: a
//       chunk over a bound is left alone (sizes[i] = 0 for the hash); a
//       candidate of the flat pass (b64_flat_candidate) takes the flat tile
//       body; anything else the encoder-layout body, which marks redo[] itself
//       for a length no encoder writes.  Text of all three peers in caller
//       order, one launch, no reorder.  One LDS stage buffer, the larger of the
//       two bodies', serves both.  The bodies are b64_decode_tiles.hpp's.
//   b64_decode_scan_kernel     one workgroup per chunk, gone at once unless
//       redo[i]: b64_update_stages.hpp's scan_stage -- the general rule of
//       b64_decode_kernel, its sextets in LDS instead of a scratch area sized
//       by a host prefix sum -- on a fresh record over the whole text, then
//       sizes/over by the one-pass contract and zeros behind a short decode.
//   lbf_sha1_launch            over the slots with d_out_sizes = min(decoded,
//       cap) as its size table: the usual kernel selection (skipped when no
//       digest or verdict is asked for).
//   b64_verify_finish_kernel   one lane per chunk: the public d_out_sizes
//       (decoded, cap + 1 when longer, UINT32_MAX over a bound) and the final
//       verdict, hash && !over && size == expected.
//
// Memory: a tile body reads the aligned 16-byte blocks that hold a byte of its
// text span and writes nothing outside out[out_off[i], + cap[i]); the scan
// reads bytes of the text only and clips every store to the slot.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "b64_decode_tiles.hpp"
#include "b64_device.hpp"
#include "b64_flat.hpp"
#include "b64_update_stages.hpp"
#include "b64_verify_launch.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

constexpr uint32_t kThreads = b64s::kThreads;
static_assert(kThreads == (uint32_t)kB64Threads, "both bodies run on 256 lanes");
constexpr uint32_t kTilesPerGroup = kDecTilesPerGroup;
static_assert(kTilesPerGroup == b64s::kFlatTilesPerGroup, "one grid for both bodies");
static_assert(kDecBytes == b64s::kTileBytes && b64s::kFlatTileText <= kDecText, "one tile of bytes; the flat text is the shorter");
// one stage buffer for both bodies, each laid over it in its own shape
constexpr uint32_t kRoutedStage = kCanonStage > b64s::kStage ? kCanonStage : b64s::kStage;

// blockIdx.x = group of tiles, blockIdx.y = chunk - chunk0.
__global__ void __launch_bounds__(kThreads) b64_decode_routed_kernel(B64VerifyLaunch p, uint32_t chunk0) {
  __shared__ uint4 stage[2 * kRoutedStage];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t last_shared;
  const uint32_t i = chunk0 + blockIdx.y, t0 = blockIdx.x * kTilesPerGroup;
  const uint32_t len = p.text_len[i], cap = p.cap[i];
  // every branch below depends on the chunk's lengths alone: the whole workgroup takes it
  if (len > p.max_text_len || cap > p.max_size) {  // not decoded; the hash reads an empty chunk
    if (t0 == 0 && threadIdx.x == 0) p.sizes[i] = 0;
    return;
  }
  if (b64_flat_candidate(len, cap)) {  // len = 4 * ceil(cap / 3) > 0, cap <= max_size <= 1 GiB: the body's preconditions
    const B64FlatDecode f{p.text, p.text_off, p.text_len, p.out, p.out_off, p.cap, p.sizes, p.over, p.redo, 0, p.n, 0};
    b64s::b64_flat_decode_tiles(f, i, t0, len, cap, reinterpret_cast<uint4(*)[b64s::kStage]>(stage), tab, last_shared);
  } else {
    b64_canon_decode_tiles(p.text, p.text_off, p.text_len, p.out, p.out_off, p.cap, p.sizes, p.over, p.redo, i, t0,
                           reinterpret_cast<uint4(*)[kCanonStage]>(stage), tab, last_shared);
  }
}

// blockIdx.x = chunk.  redo[i] is the same in every lane, and scan_stage keeps
// its barriers uniform (b64_update_stages.hpp): every barrier is reached by the
// whole workgroup.
__global__ void __launch_bounds__(kThreads) b64_decode_scan_kernel(B64VerifyLaunch p) {
  const uint32_t i = blockIdx.x;
  if (!p.redo[i]) return;  // the tile pass decoded it, or it is over a bound
  __shared__ uint4 sx[b64s::kSx / 16];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t sums[b64s::kWaves];
  __shared__ uint32_t first_eq;
  tab[threadIdx.x] = (uint8_t)b64d::value(threadIdx.x);  // published by the stage's first barrier
  const uint32_t cap = p.cap[i];
  const uint64_t slot = p.out_off[i];
  b64s::Rec r{0, 0u, 0u, false};
  b64s::scan_stage(r, b64s::Piece{p.text + p.text_off[i], p.text_len[i], p.out, slot, cap},
                   reinterpret_cast<uint8_t*>(sx), tab, sums, &first_eq);
  // an unfinished last group gives nothing (the general rule): r.decoded is the decoded length, in every lane
  const uint64_t want = r.decoded;
  if (threadIdx.x == 0) {
    p.sizes[i] = (uint32_t)min<uint64_t>(want, cap);
    p.over[i] = want > cap ? 1 : 0;
  }
  uint8_t* const o = p.out + slot;
  for (uint64_t q = want + threadIdx.x; q < cap; q += kThreads) o[q] = 0;  // never stale bytes behind a short decode
}

// One lane per chunk, behind the hash.
__global__ void __launch_bounds__(256) b64_verify_finish_kernel(B64VerifyLaunch p) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const uint32_t cap = p.cap[i];
  if (p.text_len[i] > p.max_text_len || cap > p.max_size) {
    p.sizes[i] = 0xFFFFFFFFu;
    if (p.verdicts) p.verdicts[i] = 0;
    return;
  }
  // ChunkMethods.cpp:156: the decoded length must be the chunk's size
  const bool longer = p.over[i] != 0;
  const uint32_t size = p.sizes[i];
  if (p.verdicts) p.verdicts[i] = (p.verdicts[i] && !longer && size == cap) ? 1 : 0;
  p.sizes[i] = longer ? cap + 1u : size;
}

}  // namespace

int launch_b64_verify_decode(const B64VerifyLaunch& b, hipStream_t stream) {
  if (b.n == 0) return LBF_OK;
  // the tiles of the longest text in either layout and of the largest slot
  const uint64_t tiles = std::max<uint64_t>(
      1, std::max(((uint64_t)b.max_text_len + b64s::kFlatTileText - 1) / b64s::kFlatTileText,
                  ((uint64_t)b.max_size + kDecBytes - 1) / kDecBytes));
  const uint32_t groups = (uint32_t)((tiles + kTilesPerGroup - 1) / kTilesPerGroup);
  constexpr uint32_t kPerLaunch = 65535;  // grid.y
  for (uint32_t c0 = 0; c0 < b.n; c0 += kPerLaunch) {
    hipLaunchKernelGGL(b64_decode_routed_kernel, dim3(groups, std::min(kPerLaunch, b.n - c0)), dim3(kThreads), 0,
                       stream, b, c0);
    LBF_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(b64_decode_scan_kernel, dim3(b.n), dim3(kThreads), 0, stream, b);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

int launch_b64_verify_finish(const B64VerifyLaunch& b, hipStream_t stream) {
  if (b.n == 0) return LBF_OK;
  hipLaunchKernelGGL(b64_verify_finish_kernel, dim3((b.n + 255u) / 256u), dim3(256), 0, stream, b);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace lbf

using lbf::fail;

extern "C" uint64_t lbf_b64_verify_launch_work(uint64_t n) { return 2 * n; }

extern "C" int lbf_b64_verify_launch(const char* d_text, const uint64_t* d_text_offsets, const uint32_t* d_text_lens,
                                     uint64_t n, uint32_t max_text_len, const uint32_t* d_expected_sizes,
                                     uint32_t max_size, uint8_t* d_out, const uint64_t* d_out_offsets,
                                     uint32_t* d_out_sizes, uint8_t* d_digests, const uint8_t* d_expected,
                                     uint8_t* d_verdicts, uint8_t* d_work, void* stream) {
  const std::string who = "lbf_b64_verify_launch";
  if (n == 0) return LBF_OK;
  if (!d_text || !d_text_offsets || !d_text_lens || !d_expected_sizes || !d_out || !d_out_offsets || !d_out_sizes ||
      !d_work)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  if (max_size > lbf::kVerifyLaunchMaxSize || max_text_len > lbf::kVerifyLaunchMaxText)
    return fail(LBF_ERR_INVALID, who + ": max_size or max_text_len larger than the wire decode takes (1 GiB of bytes, "
                                       "1.5 GiB of text)");
  if ((d_verdicts != nullptr) != (d_expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digest/expected arrays must be 4-byte aligned");
  const std::initializer_list<lbf::DevTable> tables = {{d_text_offsets, 8, n, "text_offsets", true},
                                                       {d_text_lens, 4, n, "text_lens", true},
                                                       {d_expected_sizes, 4, n, "expected_sizes", true},
                                                       {d_out_offsets, 8, n, "out_offsets", true},
                                                       {d_out_sizes, 4, n, "out_sizes", true},
                                                       {d_digests, 20, n, "digests", false},
                                                       {d_expected, 20, n, "expected", false},
                                                       {d_verdicts, 1, n, "verdicts", false},
                                                       {d_work, 1, 2 * n, "work", false}};
  if (int rc = lbf::tables_aligned(who, tables)) return rc;
  if (int rc = lbf::tables_fit(who, tables)) return rc;
  hipStream_t st = (hipStream_t)stream;
  LBF_HIP_TRY(hipMemsetAsync(d_work, 0, 2 * n, st));
  const lbf::B64VerifyLaunch b{reinterpret_cast<const uint8_t*>(d_text), d_text_offsets, d_text_lens, d_out,
                               d_out_offsets, d_expected_sizes, d_out_sizes, d_work, d_work + n, d_verdicts,
                               (uint32_t)n, max_text_len, max_size};
  if (int rc = lbf::launch_b64_verify_decode(b, st)) return rc;
  // the decoded lengths, clipped to the slots, are the chunk sizes the hash kernels read
  if (d_digests || d_verdicts)
    if (int rc = lbf_sha1_launch(d_out, d_out_offsets, d_out_sizes, n, d_digests, d_expected, d_verdicts, st)) return rc;
  return lbf::launch_b64_verify_finish(b, st);
}
