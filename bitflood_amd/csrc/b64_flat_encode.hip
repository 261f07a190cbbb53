// b64_flat_encode.hip -- the one-shot base64 encode of unbroken text, and the
// device-resident verify + encode launch of both layouts.
//
// bitflood's Java and Perl peers frame a chunk as RFC 4648 text without
// separators (java/com/net/BitFlood/XMLEnvelopeProcessor.java:124,
// perl/RPC/XML.pm:638): group g of the chunk, bytes [3g, 3g + 3), is characters
// [4g, 4g + 4), and a last one or two bytes are "xx==" / "xxx=".  So 12 bytes
// become one 16-character block with no line arithmetic at all, where the line
// kernel (b64_encode_kernel, kern_b64.hpp) cuts each block out of five words
// of a line's character stream.
//
//   b64_flat_encode_kernel   the line kernel's shape: tiles laid over the
//       chunk, kFlatEncTilesPerGroup consecutive tiles per workgroup, the
//       bytes staged through LDS with 16-byte loads (double-buffered when a
//       workgroup has more than one tile), each lane whole 16-character blocks
//       from one four-dword LDS window, stored with one 16-byte store; a block
//       that is not wholly inside the chunk's slot, or whose address is not
//       16-byte aligned, goes byte by byte.  grid = (groups of tiles, chunks),
//       at most 65,535 chunks per launch.  The geometry of record is one tile
//       of 6,144 bytes per workgroup (b64_flat_encode.hpp has the runs): the
//       resident workgroups of a CU overlap one another's loads, and a second
//       tile per workgroup cost 8 %.
//
//   b64_oversize_kernel      lbf_verify_encode_b64_launch sizes its grids by
//       the caller's max_size; a chunk larger than that has an incomplete
//       text, and this clears its verdict behind the hash.
//
// Memory: the bytes are read as the aligned 16-byte blocks that hold a byte of
// the tile's span (such a block lies in the span's page), at any phase; no
// byte outside text[text_off[i], + 4 * ceil(size[i] / 3)) is written, so slots
// may touch at any phase.
//
// The staging, the block store, the alphabet and a group's characters are
// b64_device.hpp's, shared with the line kernel.  DESIGN.md §4.5.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "b64_device.hpp"
#include "b64_flat_encode.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTileGroups = kFlatEncTileGroups, kTileBytes = kFlatEncTileBytes, kTileText = kFlatEncTileText;
constexpr uint32_t kTilesPerGroup = kFlatEncTilesPerGroup;
constexpr uint32_t kTileBlocks = kTileText / 16;  // 512: two per lane
#ifndef LBF_B64_FLAT_ENC_AB  // an A/B build sets the geometry's two macros and this one
// The geometry of record, as tests/wire_flat_encode_model.py states it.
static_assert(kTileBytes == 6144 && kTileText == 8192 && kTilesPerGroup == 1, "the flat encode's geometry of record");
#endif
static_assert(kTileGroups % 16 == 0, "bytes and text of a tile are whole 16-byte blocks");
// a tile's span at any phase, and slack for the last block's window: four dwords from (phase + 12 * block) / 4
constexpr uint32_t kStageBlocks = kTileBytes / 16 + 3;
static_assert(15 + 12 * (kTileBlocks - 1) + 16 <= 16 * kStageBlocks, "the window stays inside the stage");
constexpr uint32_t kPer = (kTileBytes / 16 + 1 + kThreads - 1) / kThreads;  // staged blocks per lane
// text positions within a chunk are 32-bit: the largest chunk's text and the tiles a grid may add behind it
static_assert(4ull * (b64e::kEncMaxChunk / 3 + 1) + (uint64_t)kTilesPerGroup * kTileText < (1ull << 32),
              "text positions fit 32 bits");
using b64d::put_block;
using Stage = b64d::Stage<kPer, kThreads, 0>;  // a tile's span, len > 0: at most kTileBytes / 16 + 1 blocks

// One tile of the text from its bytes in LDS (w, from byte `delta`): block u of
// the tile, characters [16u, 16u + 16), is groups 4u .. 4u + 3, the twelve
// bytes from delta + 12u.  Four aligned dwords hold them at the phase delta & 3
// (the same in every lane and every block); three v_alignbyte make them three
// dwords, and one v_perm_b32 per group its 24 bits, first byte highest.
// kWhole: every group of the tile is a whole group of the chunk (all tiles but
// a chunk's last), so none needs the end-of-text checks.
template <bool kWhole>
__device__ __forceinline__ void encode_tile(const uint32_t* w, uint32_t delta, const uint8_t* alpha, uint32_t tile,
                                            uint32_t full, uint32_t rest, uint64_t tl, uint8_t* t) {
  const uint32_t tbeg = tile * kTileText, gbeg = tile * kTileGroups, sh = delta & 3u;
  // group gg of the chunk, its three bytes in x, as its four characters, first character in the low byte
  auto chars = [&](uint32_t x, uint32_t gg) -> uint32_t {
    if (!kWhole && (gg > full || (gg == full && rest == 0))) return 0u;  // past the text: cut away by the slot's end
    return kWhole || gg < full ? b64d::chars_whole(alpha, x) : b64d::chars_last(alpha, x, rest);
  };
  for (uint32_t u = threadIdx.x; u < kTileBlocks; u += kThreads) {
    const uint32_t pos = tbeg + 16 * u;
    if (pos >= tl) break;
    const uint32_t* wb = w + ((delta + 12 * u) >> 2);
    const uint32_t w0 = wb[0], w1 = wb[1], w2 = wb[2], w3 = wb[3];
    const uint32_t d0 = __builtin_amdgcn_alignbyte(w1, w0, sh), d1 = __builtin_amdgcn_alignbyte(w2, w1, sh),
                   d2 = __builtin_amdgcn_alignbyte(w3, w2, sh);
    // selector bytes 0-3 pick from the second source, 4-7 from the first, 12 gives 0
    const uint32_t g = gbeg + 4 * u;
    const uint4 out = make_uint4(chars(__builtin_amdgcn_perm(0u, d0, 0x0C000102u), g),
                                 chars(__builtin_amdgcn_perm(d1, d0, 0x0C030405u), g + 1),
                                 chars(__builtin_amdgcn_perm(d2, d1, 0x0C020304u), g + 2),
                                 chars(__builtin_amdgcn_perm(0u, d2, 0x0C010203u), g + 3));
    put_block(t, (uint64_t)pos, (uint64_t)0, tl, out);  // clipped to the slot's end
  }
}

// blockIdx.x = group of tiles, blockIdx.y = chunk - chunk0: tile k of chunk i
// encodes bytes [6144k, +6144) into characters [8192k, +8192), clipped to the
// chunk.  Every branch around a barrier depends on the chunk's size and the
// workgroup's place alone: the whole workgroup takes it.
__global__ void __launch_bounds__(kThreads) b64_flat_encode_kernel(const uint8_t* __restrict__ data,
                                                                   const uint64_t* __restrict__ data_off,
                                                                   const uint32_t* __restrict__ size,
                                                                   uint8_t* __restrict__ text,
                                                                   const uint64_t* __restrict__ text_off,
                                                                   uint32_t chunk0) {
  constexpr uint32_t kBufs = kTilesPerGroup > 1 ? 2 : 1;  // one tile per workgroup has nothing to prefetch
  __shared__ uint4 stage[kBufs][kStageBlocks];
  __shared__ uint8_t alpha[64];
  const uint32_t i = chunk0 + blockIdx.y, t0 = blockIdx.x * kTilesPerGroup;
  const uint32_t n = size[i], full = n / 3, rest = n % 3;
  const uint64_t tl = 4ull * full + (rest ? 4 : 0);
  // the chunk's own tiles; the grid has those of the launch's max_size, so positions below stay in 32 bits
  const uint64_t own = (tl + kTileText - 1) / kTileText;
  if (t0 >= own) return;  // the whole workgroup: no barrier below is reached
  const uint32_t t1 = (uint32_t)min(own, (uint64_t)t0 + kTilesPerGroup);
  const uint8_t* d = data + data_off[i];
  uint8_t* t = text + text_off[i];
  Stage st;
  auto load = [&](uint32_t tile) {
    const uint32_t dbeg = tile * kTileBytes;
    st.clear();
    if (dbeg < n) st.load(d + dbeg, min(kTileBytes, n - dbeg));  // below n: every tile below `own` starts there
  };
  load(t0);
  b64d::fill_alphabet(alpha);
  st.store(stage[0]);
  uint32_t delta = st.delta;
  __syncthreads();
  for (uint32_t tile = t0; tile < t1; ++tile) {
    const uint32_t buf = (tile - t0) & (kBufs - 1);
    if (tile + 1 < t1) load(tile + 1);  // in flight while this tile encodes
    const uint32_t* w = reinterpret_cast<const uint32_t*>(stage[buf]);
    if ((uint64_t)(tile + 1) * kTileGroups <= full)  // uniform over the workgroup
      encode_tile<true>(w, delta, alpha, tile, full, rest, tl, t);
    else
      encode_tile<false>(w, delta, alpha, tile, full, rest, tl, t);
    if (tile + 1 < t1) {
      st.store(stage[(buf ^ 1u) & (kBufs - 1)]);  // that buffer's last reader was the previous tile, before the last barrier
      delta = st.delta;
      __syncthreads();
    }
  }
}

__global__ void __launch_bounds__(256) b64_oversize_kernel(const uint32_t* __restrict__ size, uint32_t max_size,
                                                           uint8_t* __restrict__ verdicts, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && size[i] > max_size) verdicts[i] = 0;
}

}  // namespace

int launch_b64_flat_encode(const uint8_t* data, const uint64_t* data_off, const uint32_t* size, uint8_t* text,
                           const uint64_t* text_off, uint32_t n, uint32_t max_size, hipStream_t stream) {
  if (n == 0) return LBF_OK;
  if (max_size > b64e::kEncMaxChunk) return fail(LBF_ERR_INVALID, "flat encode: max_size over 1 GiB");
  const uint64_t tl = 4 * (((uint64_t)max_size + 2) / 3);
  const uint32_t tiles = std::max<uint32_t>(1u, (uint32_t)((tl + kTileText - 1) / kTileText));
  constexpr uint32_t kPerLaunch = 65535;  // grid.y
  for (uint32_t c0 = 0; c0 < n; c0 += kPerLaunch) {
    hipLaunchKernelGGL(b64_flat_encode_kernel, dim3((tiles + kTilesPerGroup - 1) / kTilesPerGroup,
                                                    std::min(kPerLaunch, n - c0)),
                       dim3(kThreads), 0, stream, data, data_off, size, text, text_off, c0);
    LBF_HIP_TRY(hipGetLastError());
  }
  return LBF_OK;
}

}  // namespace lbf

using lbf::fail;

extern "C" int lbf_verify_encode_b64_launch(const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_sizes,
                                            uint64_t n, uint32_t max_size, uint8_t* d_digests,
                                            const uint8_t* d_expected, uint8_t* d_verdicts, int layout, char* d_text,
                                            const uint64_t* d_text_offsets, void* stream) {
  const std::string who = "lbf_verify_encode_b64_launch";
  if (int rc = lbf::check_b64_layout(who, layout)) return rc;
  if (max_size > lbf::b64e::kEncMaxChunk)
    return fail(LBF_ERR_INVALID, who + ": max_size larger than the wire encode takes (1 GiB)");
  if (n == 0) return LBF_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_text || !d_text_offsets)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  if ((d_verdicts != nullptr) != (d_expected != nullptr))
    return fail(LBF_ERR_INVALID, who + ": expected and verdicts go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_expected) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digest/expected arrays must be 4-byte aligned");
  const std::initializer_list<lbf::DevTable> tables = {{d_offsets, 8, n, "offsets", true},
                                                       {d_sizes, 4, n, "sizes", true},
                                                       {d_text_offsets, 8, n, "text_offsets", true},
                                                       {d_digests, 20, n, "digests", false},
                                                       {d_expected, 20, n, "expected", false},
                                                       {d_verdicts, 1, n, "verdicts", false}};
  if (int rc = lbf::tables_aligned(who, tables)) return rc;
  if (int rc = lbf::tables_fit(who, tables)) return rc;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* const text = reinterpret_cast<uint8_t*>(d_text);
  // the hash with the usual selection (few chains run pc4), then the layout's encode from the same bytes
  if (d_digests || d_verdicts)
    if (int rc = lbf_sha1_launch(d_data, d_offsets, d_sizes, n, d_digests, d_expected, d_verdicts, st)) return rc;
  if (int rc = lbf::launch_b64_encode_for(layout, d_data, d_offsets, d_sizes, text, d_text_offsets, (uint32_t)n, max_size,
                                          st))
    return rc;
  if (d_verdicts) {  // behind the hash on the stream: the verdict of a chunk whose text is incomplete does not stand
    hipLaunchKernelGGL(lbf::b64_oversize_kernel, dim3(((uint32_t)n + 255u) / 256u), dim3(256), 0, st, d_sizes, max_size,
                       d_verdicts, (uint32_t)n);
    LBF_HIP_TRY(hipGetLastError());
  }
  return LBF_OK;
}
