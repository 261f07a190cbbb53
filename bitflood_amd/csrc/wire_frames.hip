// wire_frames.hip -- lbf_wire_frames_launch and lbf_wire_send_chunks_launch: a
// raw receive stream resident in device memory to the tables
// lbf_b64_verify_launch reads, asynchronous on the caller's stream, with no
// host in the middle.  The host steps they restate: the '\n' split of
// FrameReader::next (host/lbf_loopback.cpp) and PeerWire::LocateSendChunk
// (host/PeerWire.cpp), which is the specification of the locate kernel.
//
//   wire_split_count_kernel    a workgroup per kSplitBlock bytes, 16 a lane read
//       as one aligned block: the '\n' among the bytes that belong to the
//       stream, counted per workgroup into d_work.
//   wire_scan_kernel           one workgroup: the exclusive prefix sum of the
//       counts in place, kScanWidth a trip with a running carry; the total is
//       *d_n_frames (split) or *d_n_located (bind).
//   wire_split_scatter_kernel  the count kernel's grid; a workgroup whose count
//       is 0 leaves without reading.  Delimiter k at position p ends frame k and
//       starts frame k + 1: p goes to d_frame_lens[k] for now, p + 1 to
//       d_frame_offsets[k + 1], and behind the last one to *d_tail.
//   wire_split_finish_kernel   a lane per frame: end - start.
//   wire_locate_kernel         a workgroup per frame.  All lanes step through
//       LocateSendChunk's grammar together; every search is one cooperative
//       primitive (16 bytes a lane, kSearchTrip a trip, minimum across the
//       workgroup).
//   wire_bind_kernel           a lane per frame: a located frame's name looked
//       up in the flood table, its chunk number into d_work.
//   wire_bind_count_kernel / wire_bind_scatter_kernel   a lane per frame: the
//       bound frames to the dense tables in frame order (count, scan, scatter).
//   wire_neutral_kernel        the dense entries behind the last bound one.
//
// No kernel waits on another workgroup and none uses an atomic: order is
// arithmetic on counts that the kernel in front completed.  Memory: of the
// stream only aligned 16-byte blocks that hold a byte of the stream (of the
// frame, in the locate kernel) are read, and bytes outside are masked out
// before they can count.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "b64_device.hpp"
#include "lbf_internal.hpp"
#include "wire_frames.hpp"

namespace lbf {
namespace wiref {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;

// 0x80 in every byte of x that equals the byte repeated in c4 (no carry crosses a byte).
__device__ __forceinline__ uint32_t eq_bytes(uint32_t x, uint32_t c4) {
  const uint32_t t = x ^ c4;
  return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t) & 0x80808080u;
}

// Bits 7, 15, 23, 31 to bits 0..3.
__device__ __forceinline__ uint32_t nibble(uint32_t h) { return (((h >> 7) * 0x00204081u) >> 21) & 0xFu; }

// Bit m set: byte m of the block is the character kChar.
template <uint32_t kChar>
__device__ __forceinline__ uint32_t hits_char(uint4 v) {
  constexpr uint32_t c4 = kChar * 0x01010101u;
  const uint32_t h0 = eq_bytes(v.x, c4), h1 = eq_bytes(v.y, c4), h2 = eq_bytes(v.z, c4), h3 = eq_bytes(v.w, c4);
  if ((h0 | h1 | h2 | h3) == 0) return 0;
  return nibble(h0) | nibble(h1) << 4 | nibble(h2) << 8 | nibble(h3) << 12;
}

// isspace() of the C locale: ' ', \t \n \v \f \r.
__device__ __forceinline__ bool is_space(uint32_t c) { return c == ' ' || c - '\t' < 5u; }

// Bit m set: byte m of the block is not white space.
__device__ __forceinline__ uint32_t hits_not_space(uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m16 = 0;
#pragma unroll
  for (uint32_t m = 0; m < 16; ++m) m16 |= (is_space((w[m >> 2] >> (8 * (m & 3))) & 255u) ? 0u : 1u) << m;
  return m16;
}

// The bytes of the block at q (q < hi) that lie in [lo, hi), as a 16-bit mask.
__device__ __forceinline__ uint32_t valid16(uint64_t q, uint64_t lo, uint64_t hi) {
  const uint32_t a = q >= lo ? 0u : (uint32_t)min((uint64_t)16, lo - q);
  const uint32_t b = (uint32_t)min((uint64_t)16, hi - q);
  return (0xFFFFu >> (16 - b)) & (0xFFFFu << a) & 0xFFFFu;
}

// A lane's delimiters: the '\n' of its 16 bytes of the split block that belong to the stream.
__device__ __forceinline__ uint32_t split_mask(const WireSplit& s, uint64_t* q_out, uint32_t* phase_out) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(s.stream);
  const uint32_t phase = (uint32_t)(a & 15u);
  const uint64_t q = (uint64_t)blockIdx.x * kSplitBlock + 16u * threadIdx.x;
  const uint64_t lo = phase, hi = (uint64_t)phase + s.stream_len;
  *q_out = q;
  *phase_out = phase;
  if (q >= hi) return 0;  // a block behind the stream is not read
  const uint4 v = *reinterpret_cast<const uint4*>(a - phase + q);
  return hits_char<'\n'>(v) & valid16(q, lo, hi);
}

__global__ void __launch_bounds__(kSplitLanes) wire_split_count_kernel(WireSplit s) {
  __shared__ uint32_t sums[kSplitLanes / 64];
  uint64_t q;
  uint32_t phase, total;
  const uint32_t m16 = split_mask(s, &q, &phase);
  b64d::wg_exclusive_scan<kSplitLanes>((uint32_t)__popc(m16), sums, &total);
  if (threadIdx.x == 0) s.counts[blockIdx.x] = total;
}

// One workgroup: counts[0, blocks) to their exclusive prefix sums, the total to
// *total.  The split's call also starts the outputs that the scatter kernel
// completes: *tail = 0 (no delimiter), and frame 0 starts at 0 if there is one.
__global__ void __launch_bounds__(kScanWidth) wire_scan_kernel(uint32_t* counts, uint32_t blocks, uint32_t* total,
                                                               uint64_t* tail, uint64_t* first_off) {
  __shared__ uint32_t sums[kScanWidth / 64];
  uint32_t carry = 0;
  for (uint32_t b0 = 0; b0 < blocks; b0 += kScanWidth) {  // the same trips in every lane
    const uint32_t b = b0 + threadIdx.x;
    const uint32_t v = b < blocks ? counts[b] : 0u;
    uint32_t trip;
    const uint32_t ex = b64d::wg_exclusive_scan<kScanWidth>(v, sums, &trip);
    if (b < blocks) counts[b] = carry + ex;
    carry += trip;
  }
  if (threadIdx.x == 0) {
    *total = carry;
    if (tail) *tail = 0;
    if (first_off && carry > 0) *first_off = 0;
  }
}

__global__ void __launch_bounds__(kSplitLanes) wire_split_scatter_kernel(WireSplit s) {
  __shared__ uint32_t sums[kSplitLanes / 64];
  const uint32_t total = *s.n_frames;
  const uint32_t base = s.counts[blockIdx.x];
  const uint32_t next = blockIdx.x + 1 < gridDim.x ? s.counts[blockIdx.x + 1] : total;
  if (next == base) return;  // no delimiter in this block: the same in every lane
  uint64_t q;
  uint32_t phase, all;
  uint32_t m16 = split_mask(s, &q, &phase);
  uint64_t k = base + b64d::wg_exclusive_scan<kSplitLanes>((uint32_t)__popc(m16), sums, &all);
  const uint64_t kept = min((uint64_t)total, (uint64_t)s.max_frames);
  while (m16) {
    const uint32_t m = (uint32_t)__ffs((int)m16) - 1u;
    m16 &= m16 - 1;
    const uint32_t p = (uint32_t)(q + m - phase);  // the delimiter's position in the stream
    if (k < kept) s.frame_len[k] = p;              // frame k's end; wire_split_finish_kernel subtracts its start
    if (k + 1 < kept) s.frame_off[k + 1] = (uint64_t)p + 1;
    if (k + 1 == total) *s.tail = (uint64_t)p + 1;
    ++k;
  }
}

__global__ void __launch_bounds__(kSplitLanes) wire_split_finish_kernel(WireSplit s) {
  const uint32_t k = blockIdx.x * kSplitLanes + threadIdx.x;
  if (k < min(*s.n_frames, s.max_frames)) s.frame_len[k] -= (uint32_t)s.frame_off[k];
}

// A tag or name of the grammar: its characters, first in the low byte of lo, and their number (<= 13).
struct Needle {
  uint64_t lo, hi;
  uint32_t n;
  __device__ __forceinline__ uint32_t at(uint32_t k) const {
    return (uint32_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 255u);
  }
};
template <uint32_t N>
constexpr Needle make_needle(const char (&lit)[N]) {
  static_assert(N - 1 <= 13, "a needle is at most 13 characters");
  Needle r{0, 0, N - 1};
  for (uint32_t k = 0; k + 1 < N; ++k)
    (k < 8 ? r.lo : r.hi) |= (uint64_t)(uint8_t)lit[k] << (8 * (k & 7));
  return r;
}
enum : uint32_t {
  kMethodName, kMethodNameEnd, kParams, kParam, kValue, kValueEnd, kParamEnd, kBase64, kString, kI4, kInt, kI4End,
  kIntEnd, kSendChunk, kLt
};
// in the order of the enum; read with scalar loads, so that no needle lives in registers between its uses
__constant__ const Needle kNeedles[] = {
    make_needle("<methodName>"), make_needle("</methodName>"), make_needle("<params>"), make_needle("<param>"),
    make_needle("<value>"),      make_needle("</value>"),      make_needle("</param>"), make_needle("<base64>"),
    make_needle("<string>"),     make_needle("<i4>"),          make_needle("<int>"),    make_needle("</i4>"),
    make_needle("</int>"),       make_needle("SendChunk"),     make_needle("<")};
__device__ __forceinline__ Needle needle_of(uint32_t id) { return kNeedles[id]; }

// ---------------------------------------------------------------------------
// One frame in the hands of its workgroup.  Every member but the lane's part of
// search() is called by all lanes with the same arguments and returns the same
// value in all of them, so the grammar below is one control flow for the
// workgroup.
// ---------------------------------------------------------------------------
struct Frame {
  const uint8_t* s;  // the frame's first byte
  uint32_t len;
  uint32_t phase;    // s mod 16
  uint32_t* slot;    // 2 x kLocateLanes / 64 words of LDS
  uint32_t par;      // which half of slot the next reduction takes

  // The smallest candidate of the workgroup, kNone when there is none.  One
  // barrier: the halves of slot alternate, and a wave reaches the next
  // reduction's barrier only after it has read this one's half.
  __device__ __forceinline__ uint32_t wg_min(uint32_t cand) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cand = min(cand, (uint32_t)__shfl_xor((int)cand, off, 64));
    uint32_t* const half = slot + par * (kLocateLanes / 64);
    if ((threadIdx.x & 63) == 0) half[threadIdx.x >> 6] = cand;
    __syncthreads();
    uint32_t r = kNone;
#pragma unroll
    for (uint32_t w = 0; w < kLocateLanes / 64; ++w) r = min(r, half[w]);
    par ^= 1u;
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)r);  // the same in every lane, and known to be
  }

  // Whether the characters of nd from the first-th on stand at p, the whole of nd inside the frame.
  __device__ __forceinline__ bool match_at(uint32_t p, const Needle& nd, uint32_t first = 0) const {
    if (p > len || nd.n > len - p) return false;
    for (uint32_t k = first; k < nd.n; ++k)
      if (s[p + k] != nd.at(k)) return false;
    return true;
  }

  // The search primitive: the first position >= from, below len, that holds no
  // white space (not_space), or at which nd stands (nd opens with '<'); kNone
  // when there is none.  Lane t of trip j takes the aligned 16-byte block
  // 256 j + t behind the one that holds `from`.
  __device__ __forceinline__ uint32_t search(uint32_t from, bool not_space, const Needle& nd) {
    if (from >= len) return kNone;
    const uint8_t* const base = s - phase;
    const uint32_t lo = from + phase, hi = len + phase;  // len <= kMaxFrame: below 2^31
    for (uint32_t q0 = lo & ~15u; q0 < hi; q0 += kSearchTrip) {  // the same trips in every lane
      const uint32_t q = q0 + 16u * threadIdx.x;
      uint32_t cand = kNone;
      if (q < hi) {
        const uint4 v = *reinterpret_cast<const uint4*>(base + q);
        uint32_t m16 = (not_space ? hits_not_space(v) : hits_char<'<'>(v)) & valid16(q, lo, hi);
        while (m16) {
          const uint32_t p = q + ((uint32_t)__ffs((int)m16) - 1u) - phase;
          if (not_space || match_at(p, nd, 1)) {
            cand = p;
            break;
          }
          m16 &= m16 - 1;
        }
      }
      const uint32_t r = wg_min(cand);
      if (r != kNone) return r;
    }
    return kNone;
  }

  // strtol(, , 10) on at most 63 characters at ws (which holds no white space),
  // then (int), then (U32).  False when no digit stands there.
  __device__ __forceinline__ bool parse_long(uint32_t ws, uint32_t* end, uint32_t* value) const {
    const uint32_t n = min(63u, len - ws);
    uint32_t k = 0;
    bool neg = false;
    if (n > 0) {
      const uint8_t c = s[ws];
      neg = c == '-';
      k = (c == '-' || c == '+') ? 1u : 0u;
    }
    const uint32_t k0 = k;
    // the magnitude saturates at LONG_MAX = 10 * kTenth + 7, or at -LONG_MIN = 10 * kTenth + 8
    constexpr uint64_t kTenth = ((1ull << 63) - 1) / 10;
    const uint32_t last = neg ? 8u : 7u;
    uint64_t acc = 0;
    bool sat = false;
    for (; k < n; ++k) {
      const uint32_t d = (uint32_t)s[ws + k] - '0';
      if (d > 9) break;
      if (acc > kTenth || (acc == kTenth && d > last))
        sat = true;
      else
        acc = acc * 10 + d;
    }
    if (k == k0) return false;
    const uint64_t x = sat ? 10 * kTenth + last : acc;
    *value = (uint32_t)(neg ? 0 - x : x);
    *end = ws + k;
    return true;
  }
};

struct Located {
  uint32_t name_off, name_len, index, text_off, text_len;  // positions in the frame
};

// PeerWire::LocateSendChunk as the steps it takes, each one search of the frame
// and what the host function does with its result; one loop, so that the
// kernel holds the search once.
enum : uint32_t {
  kFind,       // find(): false without it, else off goes behind it
  kFindName,   // ... and the method name starts there
  kFindNameEnd,  // ... and the method name that ends there is SendChunk
  kFindOpt,    // parse_value's findTag(VALUE_ETAG): behind it if it is there
  kTag,        // nextTagIs: false without it
  kTagOpt,     // nextTagIs, result unused
  kNameTag,    // getNextTag in front of a string: none, <string>, or the blank string's </value>
  kNameLt,     // stringFromXml: up to the first '<'
  kIntTag,     // getNextTag: <i4> or <int>
  kIntValue,   // intFromXml
  kIntEnd_,    // nextTagIs(</i4> or </int>)
  kTextLt      // binaryFromXml: up to the first '<'
};
struct Step {
  uint32_t op, needle;
};
__constant__ const Step kProgram[] = {
    {kFindName, kMethodName}, {kFindNameEnd, kMethodNameEnd}, {kFind, kParams},
    {kTag, kParam}, {kTag, kValue}, {kNameTag, kString}, {kNameLt, kLt}, {kFindOpt, kValueEnd}, {kTagOpt, kParamEnd},
    {kTag, kParam}, {kTag, kValue}, {kIntTag, kI4}, {kIntValue, kLt}, {kIntEnd_, kI4End}, {kFindOpt, kValueEnd},
    {kTagOpt, kParamEnd},
    {kTag, kParam}, {kTag, kValue}, {kTag, kBase64}, {kTextLt, kLt}};
__device__ __forceinline__ Step step_of(uint32_t pc) { return kProgram[pc]; }
constexpr uint32_t kSteps = 20;

__device__ __forceinline__ bool locate(Frame& f, Located* o) {
  uint32_t off = 0, mark = 0;
  bool i4 = false;
#pragma nounroll
  for (uint32_t pc = 0; pc < kSteps; ++pc) {
    const Step st = step_of(pc);
    const Needle nd = needle_of(st.op == kIntEnd_ && !i4 ? (uint32_t)kIntEnd : st.needle);
    const bool find = st.op <= kFindOpt || st.op == kNameLt || st.op == kTextLt;  // the others skip white space
    // PeerWire.cpp's find() gives up when the needle cannot fit; memchr has no such clause (nd.n is 1)
    uint32_t r = find && nd.n > f.len - min(off, f.len) ? kNone : f.search(off, !find, nd);
    if (!find && r == kNone) r = max(off, f.len);
    switch (st.op) {
      case kFind:
      case kFindName:
      case kFindNameEnd:
        if (r == kNone) return false;
        if (st.op == kFindNameEnd && (r - mark != 9 || !f.match_at(mark, needle_of(kSendChunk)))) return false;
        off = mark = r + nd.n;
        break;
      case kFindOpt:
        if (r != kNone) off = r + nd.n;
        break;
      case kTag:
      case kTagOpt:
      case kIntEnd_:
        if (f.match_at(r, nd))
          off = r + nd.n;
        else if (st.op != kTagOpt)
          return false;
        break;
      case kNameTag:  // no tag, or </value>: the string starts behind <value>, white space included
        if (r < f.len && f.s[r] == '<') {
          if (f.match_at(r, nd))
            off = r + nd.n;
          else if (!f.match_at(r, needle_of(kValueEnd)))
            return false;
        }
        mark = off;
        break;
      case kNameLt:
        if (r == kNone) return false;
        o->name_off = mark;
        o->name_len = r - mark;
        off = r;
        break;
      case kIntTag:
        i4 = f.match_at(r, nd);
        if (!i4 && !f.match_at(r, needle_of(kInt))) return false;
        off = r + (i4 ? 4 : 5);
        break;
      case kIntValue:
        if (!f.parse_long(r, &off, &o->index)) return false;
        break;
      default:  // kTextLt
        if (r == kNone) return false;
        o->text_off = off;
        o->text_len = r - off;
        break;
    }
  }
  return true;
}

// blockIdx.x = frame.
__global__ void __launch_bounds__(kLocateLanes) wire_locate_kernel(WireLocate w) {
  __shared__ uint32_t slot[2 * (kLocateLanes / 64)];
  const uint32_t i = blockIdx.x;
  if (i >= (w.live ? min(*w.live, w.n_frames) : w.n_frames)) return;  // the same in every lane
  uint64_t at = w.frame_off[i];
  const uint32_t len = w.frame_len[i];
  lbf_wire_frame out = {0, 0, 0, 0, 0, LBF_FRAME_OTHER};
  lbf_wire_frame* dst = w.frames + i;
  const uint8_t* const first = w.stream + at;
  // what only the end of the kernel needs waits in vector registers: the grammar's scalars are many
  asm volatile("" : "+v"(at), "+v"(dst));
  Located o;
  Frame f{first, len, (uint32_t)(reinterpret_cast<uintptr_t>(first) & 15u), slot, 0};
  // a frame that is too long or not inside the stream is not read
  if (len <= kMaxFrame && at <= w.stream_len && len <= w.stream_len - at && locate(f, &o)) {
    out.text_offset = at + o.text_off;
    out.name_offset = at + o.name_off;
    out.text_len = o.text_len;
    out.name_len = o.name_len;
    out.index = o.index;
    out.kind = LBF_FRAME_SEND_CHUNK_UNBOUND;
  }
  if (threadIdx.x == 0) *dst = out;
}

// A lane per frame: the file whose entry is the name as it stands in a located
// frame (the first, should two be equal), and with it the chunk.
__global__ void __launch_bounds__(kBindBlock) wire_bind_kernel(WireBind w) {
  const uint32_t i = blockIdx.x * kBindBlock + threadIdx.x;
  if (i >= w.n_frames) return;
  uint32_t chunk = kNone;
  if (i < (w.live ? *w.live : w.n_frames) && w.frames[i].kind == LBF_FRAME_SEND_CHUNK_UNBOUND) {
    const lbf_wire_frame fr = w.frames[i];
    const uint8_t* const name = w.stream + fr.name_offset;
    for (uint32_t k = 0; k < w.n_files; ++k) {
      const uint32_t n0 = w.file_name_off[k], n1 = w.file_name_off[k + 1];
      if (n1 - n0 != fr.name_len) continue;
      bool same = true;
      for (uint32_t c = 0; c < fr.name_len && same; ++c) same = w.file_names[n0 + c] == name[c];
      if (!same) continue;
      const uint32_t c0 = w.file_first[k], c1 = w.file_first[k + 1];
      if (c1 >= c0 && fr.index < c1 - c0 && c0 + fr.index < w.n_chunks) {
        chunk = c0 + fr.index;
        w.frames[i].kind = LBF_FRAME_SEND_CHUNK;
      }
      break;
    }
  }
  w.chunk[i] = chunk;
}

// blockIdx.x = group of kBindBlock frames.
__global__ void __launch_bounds__(kBindBlock) wire_bind_count_kernel(WireBind w) {
  __shared__ uint32_t sums[kBindBlock / 64];
  const uint32_t i = blockIdx.x * kBindBlock + threadIdx.x;
  const uint32_t bound = i < w.n_frames && w.chunk[i] != kNone ? 1u : 0u;
  uint32_t all;
  b64d::wg_exclusive_scan<kBindBlock>(bound, sums, &all);
  if (threadIdx.x == 0) w.counts[blockIdx.x] = all;
}

// blockIdx.x = group of kBindBlock frames; counts[] holds the groups' bases.
__global__ void __launch_bounds__(kBindBlock) wire_bind_scatter_kernel(WireBind w) {
  __shared__ uint32_t sums[kBindBlock / 64];
  const uint32_t i = blockIdx.x * kBindBlock + threadIdx.x;
  const uint32_t chunk = i < w.n_frames ? w.chunk[i] : kNone;
  uint32_t all;
  const uint64_t j =
      (uint64_t)w.counts[blockIdx.x] + b64d::wg_exclusive_scan<kBindBlock>(chunk != kNone ? 1u : 0u, sums, &all);
  if (chunk == kNone || j >= w.max_chunks) return;
  const lbf_wire_frame fr = w.frames[i];
  w.text_off[j] = fr.text_offset;
  w.text_len[j] = fr.text_len;
  w.expected_size[j] = w.chunk_sizes[chunk];
  for (uint32_t k = 0; k < 20; ++k) w.expected[20 * j + k] = w.chunk_expected[20ull * chunk + k];
  w.chunk_of[j] = chunk;
  w.frame_of[j] = i;
}

// A lane per dense entry: those behind the last bound frame decode nothing and verify as 0.
__global__ void __launch_bounds__(kBindBlock) wire_neutral_kernel(WireBind w) {
  const uint32_t j = blockIdx.x * kBindBlock + threadIdx.x;
  if (j >= w.max_chunks || j < *w.n_located) return;
  w.text_off[j] = 0;
  w.text_len[j] = 0;
  w.expected_size[j] = 0;
  for (uint32_t k = 0; k < 20; ++k) w.expected[20ull * j + k] = 0;
  w.chunk_of[j] = kNone;
  w.frame_of[j] = kNone;
}

}  // namespace

int launch_wire_split(const WireSplit& s, hipStream_t stream) {
  const uint32_t blocks = (uint32_t)split_blocks(s.stream_len);
  hipLaunchKernelGGL(wire_split_count_kernel, dim3(blocks), dim3(kSplitLanes), 0, stream, s);
  LBF_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(wire_scan_kernel, dim3(1), dim3(kScanWidth), 0, stream, s.counts, blocks, s.n_frames, s.tail,
                     s.frame_off);
  LBF_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(wire_split_scatter_kernel, dim3(blocks), dim3(kSplitLanes), 0, stream, s);
  LBF_HIP_TRY(hipGetLastError());
  const uint32_t most = std::min(s.max_frames, s.stream_len);  // a frame per byte at the most
  if (most == 0) return LBF_OK;
  hipLaunchKernelGGL(wire_split_finish_kernel, dim3((most + kSplitLanes - 1) / kSplitLanes), dim3(kSplitLanes), 0,
                     stream, s);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

int launch_wire_locate(const WireLocate& l, const WireBind& w, hipStream_t stream) {
  if (l.n_frames) {
    hipLaunchKernelGGL(wire_locate_kernel, dim3(l.n_frames), dim3(kLocateLanes), 0, stream, l);
    LBF_HIP_TRY(hipGetLastError());
  }
  const uint32_t blocks = (uint32_t)bind_blocks(w.n_frames);
  if (blocks && (w.n_files || w.max_chunks)) {
    hipLaunchKernelGGL(wire_bind_kernel, dim3(blocks), dim3(kBindBlock), 0, stream, w);
    LBF_HIP_TRY(hipGetLastError());
  }
  if (!w.max_chunks) return LBF_OK;
  if (blocks) {
    hipLaunchKernelGGL(wire_bind_count_kernel, dim3(blocks), dim3(kBindBlock), 0, stream, w);
    LBF_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(wire_scan_kernel, dim3(1), dim3(kScanWidth), 0, stream, w.counts, blocks, w.n_located,
                     (uint64_t*)nullptr, (uint64_t*)nullptr);
  LBF_HIP_TRY(hipGetLastError());
  if (blocks) {
    hipLaunchKernelGGL(wire_bind_scatter_kernel, dim3(blocks), dim3(kBindBlock), 0, stream, w);
    LBF_HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(wire_neutral_kernel, dim3((w.max_chunks + kBindBlock - 1) / kBindBlock), dim3(kBindBlock), 0,
                     stream, w);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace wiref
}  // namespace lbf

using lbf::fail;
namespace wf = lbf::wiref;

extern "C" uint64_t lbf_wire_frames_launch_work(uint64_t stream_len) { return wf::split_work_bytes(stream_len); }

extern "C" uint64_t lbf_wire_send_chunks_launch_work(uint64_t n_frames) { return wf::bind_work_bytes(n_frames); }

extern "C" int lbf_wire_frames_launch(const char* d_stream, uint64_t stream_len, uint64_t* d_frame_offsets,
                                      uint32_t* d_frame_lens, uint32_t max_frames, uint32_t* d_n_frames,
                                      uint64_t* d_tail, uint8_t* d_work, void* stream) {
  const std::string who = "lbf_wire_frames_launch";
  if (stream_len == 0) return LBF_OK;
  if (!d_stream || !d_n_frames || !d_tail || !d_work) return fail(LBF_ERR_INVALID, who + ": null argument");
  if (stream_len > 0xFFFFFFFFull) return fail(LBF_ERR_INVALID, who + ": stream_len exceeds 2^32-1 per launch");
  if ((d_frame_offsets != nullptr) != (d_frame_lens != nullptr) || (d_frame_offsets != nullptr) != (max_frames != 0))
    return fail(LBF_ERR_INVALID, who + ": frame_offsets, frame_lens and max_frames go together");
  const uint64_t kept = std::min<uint64_t>(max_frames, stream_len);  // a frame per byte at the most
  const std::initializer_list<lbf::DevTable> tables = {
      {d_stream, 1, stream_len, "stream", false},
      {d_frame_offsets, 8, kept, "frame_offsets", true},
      {d_frame_lens, 4, kept, "frame_lens", true},
      {d_n_frames, 4, 1, "n_frames", true},
      {d_tail, 8, 1, "tail", true},
      {d_work, 4, wf::split_blocks(stream_len), "work", true}};
  if (int rc = lbf::tables_aligned(who, tables)) return rc;
  if (int rc = lbf::tables_fit(who, tables)) return rc;
  const wf::WireSplit s{reinterpret_cast<const uint8_t*>(d_stream),
                        (uint32_t)stream_len,
                        d_frame_offsets,
                        d_frame_lens,
                        max_frames,
                        d_n_frames,
                        d_tail,
                        reinterpret_cast<uint32_t*>(d_work)};
  return wf::launch_wire_split(s, (hipStream_t)stream);
}

extern "C" int lbf_wire_send_chunks_launch(
    const char* d_stream, uint64_t stream_len, const uint64_t* d_frame_offsets, const uint32_t* d_frame_lens,
    uint32_t n_frames, const uint32_t* d_n_frames, const char* d_file_names, const uint32_t* d_file_name_offsets,
    const uint32_t* d_file_first, uint32_t n_files, const uint32_t* d_chunk_sizes, const uint8_t* d_chunk_expected,
    uint32_t n_chunks, lbf_wire_frame* d_frames, uint64_t* d_text_offsets, uint32_t* d_text_lens,
    uint32_t* d_expected_sizes, uint8_t* d_expected, uint32_t* d_chunk_of, uint32_t* d_frame_of, uint32_t max_chunks,
    uint32_t* d_n_located, uint8_t* d_work, void* stream) {
  const std::string who = "lbf_wire_send_chunks_launch";
  const bool table = n_files != 0;
  if ((d_file_names != nullptr) != table || (d_file_name_offsets != nullptr) != table ||
      (d_file_first != nullptr) != table || (d_chunk_sizes != nullptr) != table ||
      (d_chunk_expected != nullptr) != table || (!table && n_chunks != 0))
    return fail(LBF_ERR_INVALID, who + ": the flood table's arrays, n_files and n_chunks go together");
  if (table && n_chunks == 0) return fail(LBF_ERR_INVALID, who + ": n_files without n_chunks");
  const bool dense = max_chunks != 0;
  if ((d_text_offsets != nullptr) != dense || (d_text_lens != nullptr) != dense ||
      (d_expected_sizes != nullptr) != dense || (d_expected != nullptr) != dense || (d_chunk_of != nullptr) != dense ||
      (d_frame_of != nullptr) != dense || (d_n_located != nullptr) != dense)
    return fail(LBF_ERR_INVALID, who + ": the dense tables, max_chunks and n_located go together");
  if (n_frames > 0x7FFFFFFFu) return fail(LBF_ERR_INVALID, who + ": n_frames exceeds 2^31-1 per launch");
  if (max_chunks > 0x7FFFFFFFu) return fail(LBF_ERR_INVALID, who + ": max_chunks exceeds 2^31-1 per launch");
  if (n_frames == 0 && !dense) return LBF_OK;
  if (n_frames && (!d_stream || !d_frame_offsets || !d_frame_lens || !d_frames || !d_work))
    return fail(LBF_ERR_INVALID, who + ": null argument");
  const uint64_t nf = n_frames;
  const std::initializer_list<lbf::DevTable> tables = {
      {nf ? d_stream : nullptr, 1, stream_len, "stream", false},
      {d_frame_offsets, 8, nf, "frame_offsets", true},
      {d_frame_lens, 4, nf, "frame_lens", true},
      {d_n_frames, 4, 1, "n_frames", true},
      {d_file_name_offsets, 4, (uint64_t)n_files + 1, "file_name_offsets", true},  // the names: the caller's to place
      {d_file_first, 4, (uint64_t)n_files + 1, "file_first", true},
      {d_chunk_sizes, 4, n_chunks, "chunk_sizes", true},
      {d_chunk_expected, 20, n_chunks, "chunk_expected", false},
      {d_frames, 8, 4 * nf, "frames", true},
      {d_text_offsets, 8, max_chunks, "text_offsets", true},
      {d_text_lens, 4, max_chunks, "text_lens", true},
      {d_expected_sizes, 4, max_chunks, "expected_sizes", true},
      {d_expected, 20, max_chunks, "expected", false},
      {d_chunk_of, 4, max_chunks, "chunk_of", true},
      {d_frame_of, 4, max_chunks, "frame_of", true},
      {d_n_located, 4, 1, "n_located", true},
      {nf ? d_work : nullptr, 4, wf::bind_work_bytes(nf) / 4, "work", true}};
  if (int rc = lbf::tables_aligned(who, tables)) return rc;
  if (int rc = lbf::tables_fit(who, tables)) return rc;
  uint32_t* const work = reinterpret_cast<uint32_t*>(d_work);
  const wf::WireLocate l{reinterpret_cast<const uint8_t*>(d_stream), stream_len, d_frame_offsets, d_frame_lens,
                         n_frames, d_n_frames, d_frames};
  const wf::WireBind b{reinterpret_cast<const uint8_t*>(d_stream),
                       d_frames,
                       n_frames,
                       d_n_frames,
                       reinterpret_cast<const uint8_t*>(d_file_names),
                       d_file_name_offsets,
                       d_file_first,
                       n_files,
                       d_chunk_sizes,
                       d_chunk_expected,
                       n_chunks,
                       d_text_offsets,
                       d_text_lens,
                       d_expected_sizes,
                       d_expected,
                       d_chunk_of,
                       d_frame_of,
                       max_chunks,
                       d_n_located,
                       work,
                       nf ? work + nf : nullptr};
  return wf::launch_wire_locate(l, b, (hipStream_t)stream);
}
