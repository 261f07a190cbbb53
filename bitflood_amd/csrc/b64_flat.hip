// b64_flat.hip -- the flat path of the base64 decode: unbroken RFC 4648 text,
// 4 * ceil(size / 3) characters with '=' padding and nothing else.
//
// bitflood's three peers do not lay a chunk's base64 out the same way.
// xmlrpc++ (C++) writes lines of 72 alphabet characters and a separator, and
// kern_b64.hpp's one-pass decode and b64_update_lines.hip place every
// character by that layout.  The Java peer sends Base64.encodeToString(arg,
// false) (java/com/net/BitFlood/XMLEnvelopeProcessor.java:124, sdk/Base64.java
// with lineSep == false) and the Perl peer MIME::Base64::encode_base64($value,
// '') (perl/RPC/XML.pm:638, :671, :734): no separators at all.  For such a
// text character i is sextet i: group g is characters [4g, 4g + 4) and bytes
// [3g, 3g + 3), with no columns and no separator places.  Two kernels:
//
//   b64_flat_decode_kernel   the one-shot pass of lbf_b64_verify_batch, for
//       chunks whose text length is the unbroken text's and not the encoder's.
//       The one-pass decode's shape (kern_b64.hpp): tiles of 3,888 bytes = 243
//       blocks of 16 from 5,184 characters, four tiles per workgroup -- the
//       geometry that kernel's A/B runs settled on (72-line tiles, 243 of 256
//       lanes busy, four tiles per workgroup: profiles/r05/b64_geometry/) --
//       text double-buffered in LDS, each lane one block from one LDS window.
//       A text that is not flat (junk, '=' anywhere but "xx==" / "xxx=" in the
//       last group) is marked in redo[] and decoded again by the general
//       kernel, whose rule gives the same bytes on every flat text.
//
//   b64_update_flat_kernel   the piecewise pass of lbf_b64_update_launch,
//       between b64_update_lines_kernel and b64_update_kernel, one workgroup
//       per piece.  It takes the longest prefix of what the line kernel left
//       that it can show to be flat, a tile at a time: the carried group
//       completed from the next 4 - ncarry characters, then whole groups of
//       alphabet characters up to one that holds '='.  The prefix ends behind
//       a group, so nothing is carried.  Tiles are laid over the CHUNK (block u
//       of tile k holds chunk bytes [3888k + 16u, +16)), so a piece's first and
//       last tile are partial and a block that is not wholly the piece's is
//       written by bytes.  A tile is validated before it is stored; one with a
//       character outside the alphabet writes nothing and ends the prefix at
//       its start.  The kernel never finalises a chain.  tests/wire_flat_model.py
//       restates the rule and tests/test_b64_flat_cpu.py holds it to the
//       general one.
//
// The staging, the table entry, the window and the packing are
// b64_device.hpp's; the tile's geometry and the piecewise stage itself
// (flat_stage) are b64_update_stages.hpp's, which the fused kernel
// (b64_update_fused.hip) uses too.  DESIGN.md §4.7.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "b64_decode_tiles.hpp"
#include "b64_device.hpp"
#include "b64_flat.hpp"
#include "b64_update_stages.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

using namespace b64s;

// The tile of both kernels is b64_update_stages.hpp's: kTileBytes = 3888 bytes (243 blocks of 16, 1,296 groups)
// from kTileText = 5184 characters.
constexpr uint32_t kTileText = kFlatTileText;
static_assert(kTileBytes == 3888 && kTileText == 5184, "the tile as stated above and in tests/wire_flat_model.py");
constexpr uint32_t kTilesPerGroup = kFlatTilesPerGroup;  // the one-shot pass: consecutive tiles of a chunk per workgroup

// ---------------------------------------------------------------------------
// The one-shot pass.  blockIdx.x = group of tiles, blockIdx.y = chunk -
// chunk0.  Chunk i's text is text[text_off[i] .. + text_len[i]), text_len[i] =
// 4 * ceil(cap[i] / 3): G = text_len / 4 groups, the last of them "xxxx",
// "xxx=" or "xx==".  Tile k reads characters [5184k, +5184) and writes bytes
// [3888k, +3888), so the text's tiles cover the slot.  out[out_off[i] .. +
// cap[i]): the decoded bytes, zeros behind a short decode, nothing at or past
// cap.  sizes[i] = min(decoded, cap[i]), over[i] = decoded > cap[i] (the
// one-pass decode's contract, kern_b64.hpp).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) b64_flat_decode_kernel(B64FlatDecode b) {
  __shared__ uint4 stage[2][kStage];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t last_shared;
  const uint32_t i = b.chunk0 + blockIdx.y, t0 = blockIdx.x * kTilesPerGroup;
  const uint32_t len = b.text_len[i], limit = b.cap[i];
  // the host routes candidates only; any other length is the general decode's (the whole workgroup leaves)
  if (len == 0 || limit > kMaxCap || (uint64_t)len != 4 * (((uint64_t)limit + 2) / 3)) {
    if (t0 == 0 && threadIdx.x == 0) b.redo[i] = 1;
    return;
  }
  const uint32_t groups = len / 4;
  const uint32_t own = (len + kTileText - 1) / kTileText;
  if (t0 >= own) return;  // the whole workgroup: no barrier below is reached
  const uint32_t t1 = min(own, t0 + kTilesPerGroup);
  const uint8_t* const t = b.text + b.text_off[i];
  uint8_t* const o = b.out + b.out_off[i];
  const uint32_t delta = 16 * kPad + (uint32_t)(reinterpret_cast<uintptr_t>(t) & 15u);  // of every tile: 5,184 = 16 * 324
  Stage st;
  auto load = [&](uint32_t tile) {
    const uint32_t tbeg = tile * kTileText;  // below len
    st.load(t + tbeg, min(kTileText, len - tbeg));
  };
  load(t0);
  tab[threadIdx.x] = (uint8_t)value(threadIdx.x);
  if (threadIdx.x == 0) {
    // the last group -- "xxxx", "xxx=" or "xx==" -- sets the decoded length
    const uint32_t at = 4 * (groups - 1);
    const uint32_t c2 = value(t[at + 2]), c3 = value(t[at + 3]);
    const uint32_t last = c3 < 64 ? 3u : c2 < 64 ? 2u : 1u;
    last_shared = last;
    if (t0 == 0) {
      const uint64_t want = 3ull * (groups - 1) + last;
      b.sizes[i] = (uint32_t)min<uint64_t>(want, limit);
      b.over[i] = want > limit ? 1 : 0;
      if (c3 == kSkip || c2 == kSkip || (c2 == kEq && c3 != kEq)) b.redo[i] = 1;
    }
  }
  st.store(stage[0]);
  __syncthreads();
  const uint32_t want = 3 * (groups - 1) + last_shared;  // at most 2^30 + 2
  bool bad = false;
  for (uint32_t tile = t0; tile < t1; ++tile) {
    const uint32_t buf = (tile - t0) & 1u;
    if (tile + 1 < t1) load(tile + 1);  // in flight while this tile decodes
    const uint32_t b0 = 16 * threadIdx.x, pos = tile * kTileBytes + b0;
    if (threadIdx.x < kTileBlocks && pos < limit) {
      const uint32_t g0 = b0 / 3, phase = b0 - 3 * g0;
      uint32_t x[6], inner, head;
      six_groups(reinterpret_cast<const uint8_t*>(stage[buf]), delta + 4 * g0, tab, x, &inner, &head);
      // window groups j < rel lie in front of the chunk's last group (all four characters of the alphabet);
      // group rel is the last (its first two of the alphabet; lane 0 checked its padding); those behind
      // it were decoded from whatever lay in LDS, and their bytes lie at or past `want`
      const int32_t rel = (int32_t)groups - 1 - (int32_t)(tile * kTileGroups + g0);  // >= 0: pos < limit <= 3 * groups
      const uint32_t nin = (uint32_t)min(rel, 6);
      const uint32_t head_mask = rel < 6 ? 3u << (2 * rel) : 0u;
      bad |= ((inner & ((1u << (2 * nin)) - 1u)) | (head & head_mask)) != 0;
      uint4 v = pack16(x, phase);
      if (pos + 16 > want) v = zero_from(v, want > pos ? want - pos : 0u);  // zeros behind a short decode
      put_block(o + pos, v, 0u, limit - pos);
    }
    if (tile + 1 < t1) {
      st.store(stage[buf ^ 1u]);  // that buffer's last reader was the previous tile, before the last barrier
      __syncthreads();
    }
  }
  if (bad) b.redo[i] = 1;  // every writer stores the same 1
}

// ---------------------------------------------------------------------------
// The piecewise pass.  blockIdx.x = piece.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) b64_update_flat_kernel(B64FlatParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written, the hand-off included
  __shared__ uint4 stage[2][kStage];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t wave_bad[2][kWaves];

  uint8_t* const rec = p.b64_states + 16 * si;
  Rec r = read_rec(rec);
  const uint64_t decoded = r.decoded;
  const uint32_t cap = p.cap[i], piece_len = p.text_len[i];
  uint32_t skip = 0;  // the characters the line kernel took
  if (p.after_lines) {
    skip = p.taken[i];
    if (skip > piece_len) skip = piece_len;  // never: the line path takes a prefix
  }
  uint32_t took = 0;
  // a chunk or a record the batch call would refuse, or no text left: the rest is b64_update_kernel's whole (the
  // whole workgroup: every value is the same in every lane)
  if (cap <= kMaxCap && !nothing_to_take(r, piece_len - skip)) {
    tab[threadIdx.x] = (uint8_t)value(threadIdx.x);
    const Piece pc{p.text + p.text_off[i] + skip, piece_len - skip, p.out, p.out_off[i], cap};
    took = flat_stage(r, pc, stage, tab, wave_bad);
  }
  if (threadIdx.x == 0) {
    if (r.decoded != decoded) *reinterpret_cast<uint4*>(rec) = rec_words(r);  // behind a group: nothing is carried
    if (!p.after_lines) {
      p.before[i] = decoded;
      p.taken[i] = took;
    } else if (took) {  // behind the line kernel both entries are written already
      p.taken[i] = skip + took;
    }
    if (p.flat_chars) p.flat_chars[i] = took;
  }
}

}  // namespace

// grid = (groups of kTilesPerGroup tiles, chunks), in launches of at most 65,535 chunks (grid.y)
int launch_b64_flat_decode(const B64FlatDecode& b, hipStream_t stream) {
  if (b.n == 0) return LBF_OK;
  const uint32_t tiles = std::max(1u, (b.max_text_len + kTileText - 1) / kTileText);
  constexpr uint32_t kPerLaunch = 65535;
  for (uint32_t c0 = 0; c0 < b.n; c0 += kPerLaunch) {
    B64FlatDecode s = b;
    s.chunk0 = b.chunk0 + c0;
    s.n = std::min(kPerLaunch, b.n - c0);
    hipLaunchKernelGGL(b64_flat_decode_kernel, dim3((tiles + kTilesPerGroup - 1) / kTilesPerGroup, s.n), dim3(kThreads),
                       0, stream, s);
    LBF_HIP_TRY(hipGetLastError());
  }
  return LBF_OK;
}

int launch_b64_update_flat(const B64FlatParams& p, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(b64_update_flat_kernel, dim3(n), dim3(kThreads), 0, stream, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace lbf

// The flat path's switch: LBF_B64_FLAT at first use, then lbf_set_b64_flat.
static std::atomic<int> g_b64_flat{-1};

bool lbf::b64_flat_enabled() {
  int v = g_b64_flat.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("LBF_B64_FLAT");
    const int from_env = lbf::kB64FlatDefault ? !(e && e[0] == '0' && e[1] == 0) : (e && e[0] == '1' && e[1] == 0);
    g_b64_flat.compare_exchange_strong(v, from_env, std::memory_order_relaxed);  // a setter that got in first wins
    v = g_b64_flat.load(std::memory_order_relaxed);
  }
  return v != 0;
}

extern "C" int lbf_set_b64_flat(int on) {
  const int before = lbf::b64_flat_enabled() ? 1 : 0;
  g_b64_flat.store(on ? 1 : 0, std::memory_order_relaxed);
  return before;
}
