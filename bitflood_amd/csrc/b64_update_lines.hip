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
// What it needs of kern_b64.hpp (the staging, the table entry, the block) is
// restated here, as b64_update.hip restates the table.
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "b64_update_lines.hpp"
#include "lbf_internal.hpp"

namespace lbf {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxCap = 1u << 30;        // the wire calls' bound on a chunk
constexpr uint64_t kMaxDecoded = 1ull << 61;  // b64_update_kernel's clamp
constexpr uint32_t kEq = 64, kSkip = 255;
constexpr uint32_t kTileLines = 72;
constexpr uint32_t kTileText = kTileLines * 73, kTileBytes = kTileLines * 54, kTileGroups = kTileLines * 18;
constexpr uint32_t kTileBlocks = kTileBytes / 16;  // 243
static_assert(kTileBytes % 16 == 0 && kTileBlocks <= kThreads, "one 16-byte block per lane");
// A tile's text is staged as the aligned 16-byte blocks that hold it, behind
// kPad blocks: the first block of a piece reads its six-group window from up to
// 24 characters in front of the piece's first group (masked, but read).
constexpr uint32_t kPad = 2;
constexpr uint32_t kSpan = (kTileText + 15 + 15) / 16;  // 330 blocks: a tile at any phase
constexpr uint32_t kStage = kPad + kSpan + 2;           // and slack for the last window's 32-byte read
constexpr uint32_t kPer = (kSpan + kThreads - 1) / kThreads;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static_assert(sizeof(lbf_b64_state) == 16 && offsetof(lbf_b64_state, decoded) == 0 &&
                  offsetof(lbf_b64_state, carry) == 8 && offsetof(lbf_b64_state, ncarry) == 12 &&
                  offsetof(lbf_b64_state, ended) == 13,
              "lbf_b64_state layout");

// The decode table entry of character c: 0..63, kEq for '=', kSkip otherwise.
__device__ __forceinline__ uint32_t value(uint32_t c) {
  return c - 'A' < 26u ? c - 'A' : c - 'a' < 26u ? c - 'a' + 26 : c - '0' < 10u ? c - '0' + 52 :
         c == '+' ? 62u : c == '/' ? 63u : c == '=' ? kEq : kSkip;
}

// Global bytes [src, src + len) into LDS as the aligned 16-byte blocks that
// hold them (a block that holds one byte of the span lies in its page): LDS
// byte 16 * kPad + (src mod 16) + k = src[k].  load() issues the loads, store()
// waits for them, so the tile in hand decodes while the next one's text flies.
struct Stage {
  u32x4 v[kPer];
  uint32_t blocks = 0;
  __device__ __forceinline__ void load(const uint8_t* src, uint32_t len) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const uint32_t phase = (uint32_t)(a & 15u);
    const u32x4* g = reinterpret_cast<const u32x4*>(a - phase);
    blocks = (phase + len + 15) / 16;  // at most kSpan
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (threadIdx.x + k * kThreads < blocks) v[k] = __builtin_nontemporal_load(g + threadIdx.x + k * kThreads);
  }
  __device__ __forceinline__ void store(uint4* lds) const {
    u32x4* l = reinterpret_cast<u32x4*>(lds) + kPad;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (threadIdx.x + k * kThreads < blocks) l[threadIdx.x + k * kThreads] = v[k];
  }
};

// The lane's block of a tile: bytes [16 * lane, +16) of the tile from its six
// groups g0 .. g0 + 5 (kern_b64.hpp's b64_decode_block), of which only groups
// [gl, gh) of the tile are this piece's.  Character c of the tile is LDS byte
// delta + c.  *bad is set when one of the piece's groups holds a character
// outside the alphabet, or a separator place between two of its groups (up to
// group sep_hi - 1) holds one of the alphabet or '='.  Bytes of groups outside
// [gl, gh) are whatever lay in LDS; the caller stores none of them.
__device__ __forceinline__ uint4 decode_block(const uint8_t* sb, uint32_t delta, const uint8_t* tab, uint32_t gl,
                                              uint32_t gh, uint32_t sep_hi, bool* bad) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(sb);
  const uint32_t b0 = 16 * threadIdx.x, g0 = b0 / 3, phase = b0 - 3 * g0;
  const uint32_t l0 = g0 / 18, r0 = g0 - 18 * l0;
  const uint32_t c0 = delta + 4 * g0 + l0, sh0 = c0 & 3u;
  const uint32_t* wb = w + (c0 >> 2);
  uint32_t win[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) win[k] = wb[k];
  uint32_t x[6];
  uint32_t flags = 0;  // two bits per group, at 2j: zero exactly when its four characters are of the alphabet
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const uint32_t sep = r0 + j >= 18 ? 1u : 0u;
    const uint32_t off = sh0 + sep;  // 0..4: the group's offset from dword j of the window
    const uint32_t lo = off >= 4 ? win[j + 1] : win[j], hi = off >= 4 ? win[j + 2] : win[j + 1];
    const uint32_t c = __builtin_amdgcn_alignbyte(hi, lo, off & 3u);
    const uint32_t s0 = tab[c & 255], s1 = tab[(c >> 8) & 255], s2 = tab[(c >> 16) & 255], s3 = tab[c >> 24];
    flags |= ((s0 | s1 | s2 | s3) >> 6) << (2 * j);
    x[j] = (((s0 << 6) | s1) << 12) | ((s2 << 6) | s3);  // unmasked: a flagged group's bytes are never stored
  }
  const uint32_t jl = gl > g0 ? gl - g0 : 0u, jh = gh - g0 < 6u ? gh - g0 : 6u;  // g0 < gh, jl < 6: the caller's test
  const uint32_t mask = ((1u << (2 * jh)) - 1u) & ~((1u << (2 * jl)) - 1u);
  bool b = (flags & mask) != 0;
  if (r0 >= 12) {  // the line's separator follows window group 17 - r0
    const uint32_t js = 17 - r0, gs = g0 + js;
    if (gs >= gl && gs + 1 < sep_hi) b |= tab[sb[c0 + 4 * js + 4]] != kSkip;
  }
  *bad = b;
  // the 18 bytes of the six groups as little-endian words: group j's bytes are
  // x[j]'s bytes 2, 1, 0 (selector bytes 0-3 pick from the second source, 4-7
  // from the first, 12 gives 0)
  const uint32_t W0 = __builtin_amdgcn_perm(x[1], x[0], 0x06000102u);
  const uint32_t W1 = __builtin_amdgcn_perm(x[2], x[1], 0x05060001u);
  const uint32_t W2 = __builtin_amdgcn_perm(x[3], x[2], 0x04050600u);
  const uint32_t W3 = __builtin_amdgcn_perm(x[5], x[4], 0x06000102u);
  const uint32_t W4 = __builtin_amdgcn_perm(x[5], x[5], 0x0C0C0001u);
  return make_uint4(__builtin_amdgcn_alignbyte(W1, W0, phase), __builtin_amdgcn_alignbyte(W2, W1, phase),
                    __builtin_amdgcn_alignbyte(W3, W2, phase), __builtin_amdgcn_alignbyte(W4, W3, phase));
}

// blockIdx.x = piece.
__global__ void __launch_bounds__(kThreads) b64_update_lines_kernel(B64LinesParams p) {
  const uint32_t i = blockIdx.x;
  const uint64_t si = p.state_of ? (uint64_t)p.state_of[i] : (uint64_t)i;
  if (si >= p.n_states) return;  // names no chain: nothing is read or written, the hand-off included
  __shared__ uint4 stage[2][kStage];
  __shared__ uint8_t tab[256];
  __shared__ uint32_t wave_bad[2][kThreads / 64];

  uint8_t* const rec = p.b64_states + 16 * si;
  const uint4 r = *reinterpret_cast<const uint4*>(rec);
  uint64_t decoded = (uint64_t)r.x | ((uint64_t)r.y << 32);
  if (decoded > kMaxDecoded) decoded = kMaxDecoded;  // b64_update_kernel's clamps, all three
  const uint32_t nc = r.w & 3u;
  const uint32_t carry = r.z & ((1u << (6u * nc)) - 1u);
  const bool ended = ((r.w >> 8) & 0xFFu) != 0;
  const uint32_t cap = p.cap[i], len = p.text_len[i];
  // a record the batch call would refuse, or nothing to take: the piece is b64_update_kernel's whole
  if (cap > kMaxCap || ended || decoded % 3 != 0 || len == 0) {
    if (threadIdx.x == 0) {
      p.before[i] = decoded;
      p.taken[i] = 0;
      if (p.line_chars) p.line_chars[i] = 0;
    }
    return;  // the whole workgroup: every value above is the same in every lane
  }
  const uint8_t* const t = p.text + p.text_off[i];
  const uint64_t slot = p.out_off[i];  // positions are sums of 64-bit numbers, taken mod 2^64
  tab[threadIdx.x] = (uint8_t)value(threadIdx.x);

  // ---- the head: the carried group, the separator at column 0.  Every lane
  // ---- works it out; lane 0 writes.
  uint64_t D = decoded;  // bytes of the chain decoded so far; a multiple of 3 from here on
  uint32_t pos = 0;      // characters of the piece taken so far
  bool go = true;
  if (nc != 0) {
    const uint32_t need = 4 - nc;
    uint32_t x = 0, junk = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k)
      if (k < nc) x |= ((carry >> (6u * k)) & 63u) << (18u - 6u * k);
    if (len < need) {
      go = false;
    } else {
#pragma unroll
      for (uint32_t k = 1; k < 4; ++k) {
        if (k < nc) continue;
        const uint32_t v = value(t[k - nc]);
        junk |= v >> 6;
        x |= (v & 63u) << (18u - 6u * k);
      }
      go = junk == 0;
    }
    if (go) {
      if (threadIdx.x == 0) {
        uint8_t* const o = p.out + (slot + D);
        if (D < cap) o[0] = (uint8_t)(x >> 16);
        if (D + 1 < cap) o[1] = (uint8_t)(x >> 8);
        if (D + 2 < cap) o[2] = (uint8_t)x;
      }
      D += 3;  // at most 2^61 + 1: no wrap
      pos = need;
    }
  }
  uint32_t groups = 0;  // whole groups that follow, by the piece's length
  uint32_t col = 0;     // groups into the line
  if (go) {
    col = (uint32_t)((D / 3) % 18);
    bool sep_missing = false;
    if (col == 0 && pos < len) {
      if (value(t[pos]) == kSkip)
        ++pos;  // the separator, whether or not S is 0
      else
        sep_missing = nc != 0;  // the carried group ended a line: a separator follows it, or the piece's end
    }
    const uint32_t left = len - pos, n0 = 18 - col;  // n0 groups end the line in hand; then a separator and 72 a line
    if (sep_missing) {
      groups = 0;
    } else if (left < 4 * n0) {
      groups = left / 4;
    } else {
      const uint32_t more = left - 4 * n0, q = more / 73, rem = more - 73 * q;
      groups = n0 + 18 * q + (rem ? (rem - 1) / 4 : 0u);
    }
    if (groups) {  // '=' stops the prefix: only the last group of an encoder's text holds it
      const uint32_t k = groups - 1;
      const uint8_t* const g = t + pos + 4 * k + (k + col) / 18;
      if (g[0] == '=' || g[1] == '=' || g[2] == '=' || g[3] == '=') --groups;
    }
  }

  // ---- the tiles of the chunk that hold groups [D / 3, D / 3 + groups)
  uint32_t done = 0;  // groups of validated tiles
  if (groups) {
    const uint64_t tile0 = D / kTileBytes;
    const uint32_t g_first = (uint32_t)(D - tile0 * kTileBytes) / 3;  // the first group's index in its tile
    const uint32_t c_first = 4 * g_first + g_first / 18;              // and its first character's
    const uint32_t g_end = g_first + groups;                          // < 2^30 + 1,296
    const uint32_t ntiles = (g_end + kTileGroups - 1) / kTileGroups;
    Stage st;
    uint32_t delta_next = 0;
    // tile j's groups [gl, gh) and its characters [clo, chi): its groups', the separators between them, and the
    // one behind its last group when the next tile goes on
    auto load = [&](uint32_t j) {
      const uint32_t gl = j == 0 ? g_first : 0u;
      const uint32_t gh = g_end - j * kTileGroups < kTileGroups ? g_end - j * kTileGroups : kTileGroups;
      const uint32_t more = j + 1 < ntiles ? 1u : 0u;
      const uint32_t clo = 4 * gl + gl / 18, chi = 4 * gh + (gh - 1) / 18 + more;
      // piece character of tile character c: pos + (j * kTileText + c) - c_first
      const uint8_t* const src = t + pos + ((uint64_t)j * kTileText + clo - c_first);
      st.load(src, chi - clo);
      delta_next = 16 * kPad + (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u) - clo;  // mod 2^32
    };
    load(0);
    st.store(stage[0]);
    uint32_t delta = delta_next;
    __syncthreads();  // the table and tile 0's text
    for (uint32_t j = 0; j < ntiles; ++j) {
      const uint32_t buf = j & 1u;
      const bool next = j + 1 < ntiles;
      if (next) load(j + 1);  // in flight while this tile decodes
      const uint32_t gl = j == 0 ? g_first : 0u;
      const uint32_t gh = g_end - j * kTileGroups < kTileGroups ? g_end - j * kTileGroups : kTileGroups;
      const uint32_t b0 = 16 * threadIdx.x;
      // the lanes whose block holds a byte of groups [gl, gh)
      const bool mine = threadIdx.x < kTileBlocks && b0 + 16 > 3 * gl && b0 < 3 * gh;
      bool bad = false;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (mine)
        v = decode_block(reinterpret_cast<const uint8_t*>(stage[buf]), delta, tab, gl, gh, gh + (next ? 1u : 0u), &bad);
      const bool wave_has = __ballot(bad) != 0;
      if ((threadIdx.x & 63u) == 0) wave_bad[buf][threadIdx.x >> 6] = wave_has ? 1u : 0u;
      if (next) {
        st.store(stage[buf ^ 1u]);  // that buffer's last readers were the previous tile's lanes, before its barrier
        delta = delta_next;
      }
      __syncthreads();  // the flags of this tile, the text of the next
      // (wave_bad[buf] is written again two tiles on, behind the next tile's barrier)
      if (wave_bad[buf][0] | wave_bad[buf][1] | wave_bad[buf][2] | wave_bad[buf][3]) break;  // the whole workgroup
      done += gh - gl;
      if (!mine) continue;
      // the tile is good: the block's bytes that are the piece's and lie below cap
      const uint64_t tb = (tile0 + j) * kTileBytes;  // at most 2^61 + 3,888
      const uint32_t in_cap = cap > tb ? (cap - tb < kTileBytes ? (uint32_t)(cap - tb) : kTileBytes) : 0u;
      const uint32_t wlo = 3 * gl, whi = 3 * gh < in_cap ? 3 * gh : in_cap;
      uint8_t* const o = p.out + (slot + tb + b0);
      if (b0 >= wlo && b0 + 16 <= whi && (reinterpret_cast<uintptr_t>(o) & 15u) == 0) {
        *reinterpret_cast<uint4*>(o) = v;
      } else {
        const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t m = 0; m < 16; ++m)
          if (b0 + m >= wlo && b0 + m < whi) o[m] = (uint8_t)(ws[m >> 2] >> (8 * (m & 3)));
      }
    }
  }
  if (threadIdx.x != 0) return;
  // the characters behind `pos` that the done groups and the separators between them take
  const uint32_t taken = !go ? 0u : done ? pos + 4 * done + (done - 1 + col) / 18 : pos;
  const uint64_t now = D + 3ull * done;
  if (go && now != decoded)  // the prefix ends behind a group: nothing is carried
    *reinterpret_cast<uint4*>(rec) = make_uint4((uint32_t)(now < kMaxDecoded ? now : kMaxDecoded),
                                                (uint32_t)((now < kMaxDecoded ? now : kMaxDecoded) >> 32), 0u, 0u);
  p.before[i] = decoded;
  p.taken[i] = taken;
  if (p.line_chars) p.line_chars[i] = taken;
}

}  // namespace

int launch_b64_update_lines(const B64LinesParams& p, uint32_t n, hipStream_t stream) {
  hipLaunchKernelGGL(b64_update_lines_kernel, dim3(n), dim3(kThreads), 0, stream, p);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace lbf
