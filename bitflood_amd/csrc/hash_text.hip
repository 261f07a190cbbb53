// hash_text.hip -- lbf_sha1_hashes_launch and lbf_verify_hashes_launch: chunks
// resident in device memory to and against the flood file's hash strings (the
// unpadded base64 of the SHA-1, 27 characters), asynchronous on the caller's
// stream, with no host in the middle.  Encoder::EncodeFile writes the strings;
// Flood::_SetupFilesAndChunks (Flood.cpp:259-285) compares them as strings,
// sets m_chunkmap and collects the chunks to download.
//
//   lbf_sha1_launch            the digests, into d_digests or d_work: the usual
//       kernel selection.
//   hash_text_encode_kernel    (hashes launch) one lane per chunk, 256 a
//       workgroup: five dwords of digest -> 27 characters.  Packed slots: the
//       workgroup's strings are one span of 256 x 27 bytes, assembled in LDS at
//       the span's phase in its first 16-byte block and stored as aligned
//       16-byte blocks, bytes only where a block reaches past the span.  With
//       slot offsets each lane stores its own slot: bytes up to the first
//       aligned dword, six dwords, bytes behind them.
//   hash_text_compare_kernel   (verify launch) one lane per chunk, kMapBlock a
//       workgroup: the 27 characters of the digest in registers against the
//       given string, read as the aligned dwords that hold it; the chunkmap
//       character; the workgroup's count of '0' (ballot + popcount per wave,
//       LDS across waves) into d_work.
//   hash_text_scan_kernel      one workgroup: the exclusive prefix sum of the
//       counts in place, kScanWidth a trip with a running carry; the total is
//       *d_missing_count.
//   hash_text_scatter_kernel   the compare kernel's grid: a lane whose
//       character is '0' stores its index at the workgroup's base + the '0' of
//       the waves and lanes before it.
//
// No kernel waits on another workgroup: the order of the list is arithmetic on
// counts that the kernel in front completed.  Memory: the encode kernel writes
// nothing outside the slots; the compare kernel reads, of the strings, only
// aligned dwords that hold a byte of a 27-byte string (same page as that byte).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "b64_device.hpp"
#include "hash_text.hpp"
#include "lbf_internal.hpp"

namespace lbf {
namespace htext {

namespace {

// The 27 characters of the digest at dg (4-byte aligned), four to a word, first
// character in the low byte: c[0..5] the six whole groups, c[6] the last two
// bytes' three characters with '=' above them.
__device__ __forceinline__ void digest_chars(const uint8_t* alpha, const uint8_t* dg, uint32_t c[7]) {
  const uint32_t* d = reinterpret_cast<const uint32_t*>(dg);
  uint32_t w[6];
#pragma unroll
  for (int k = 0; k < 5; ++k) w[k] = __builtin_bswap32(d[k]);  // digest bytes 4k.. from the top
  w[5] = 0;
#pragma unroll
  for (int g = 0; g < 7; ++g) {
    const int k = (24 * g) >> 5, r = (24 * g) & 31;
    const uint64_t two = (uint64_t)w[k] << 32 | w[k + 1];
    const uint32_t x = (uint32_t)(two >> (40 - r)) & 0xFFFFFFu;  // bytes 3g, 3g+1, 3g+2, first highest
    c[g] = g < 6 ? b64d::chars_whole(alpha, x) : b64d::chars_last(alpha, x, 2);
  }
}

// The 27 characters to dst at any alignment: the bytes in front of the first
// aligned dword, six dwords, the bytes behind them (27 = lead + 24 + (3 - lead)).
__device__ __forceinline__ void store_slot(uint8_t* dst, const uint32_t c[7]) {
  const uint32_t lead = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
#pragma unroll
  for (uint32_t m = 0; m < 3; ++m)
    if (m < lead) dst[m] = (uint8_t)(c[0] >> (8 * m));
  uint32_t* q = reinterpret_cast<uint32_t*>(dst + lead);
#pragma unroll
  for (int j = 0; j < 6; ++j) q[j] = __builtin_amdgcn_alignbyte(c[j + 1], c[j], lead);
  const uint32_t tail = c[6] >> (8 * lead);  // characters 24 + lead onwards
#pragma unroll
  for (uint32_t m = 0; m < 3; ++m)
    if (m + lead < 3) dst[lead + 24 + m] = (uint8_t)(tail >> (8 * m));
}

constexpr uint32_t kSpan = kEncBlock * kHashChars;      // a workgroup's packed strings
constexpr uint32_t kSpanBlocks = (kSpan + 15 + 15) / 16;  // at any phase

// blockIdx.x = group of kEncBlock chunks.  hash_off is a kernel argument: the
// whole grid takes one mode.
__global__ void __launch_bounds__(kEncBlock) hash_text_encode_kernel(const uint8_t* digests, uint8_t* hashes,
                                                                     const uint64_t* hash_off, uint32_t n) {
  __shared__ uint4 span[kSpanBlocks];
  __shared__ uint8_t alpha[64];
  b64d::fill_alphabet(alpha);
  __syncthreads();
  const uint32_t first = blockIdx.x * kEncBlock, i = first + threadIdx.x;
  const bool valid = i < n;
  uint32_t c[7];
  if (valid) digest_chars(alpha, digests + 20ull * i, c);
  if (hash_off) {
    if (valid) store_slot(hashes + hash_off[i], c);
    return;
  }
  const uint32_t len = kHashChars * min(kEncBlock, n - first);
  uint8_t* const base = hashes + (uint64_t)kHashChars * first;
  const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(base) & 15u);
  if (valid) {
    uint8_t* s = reinterpret_cast<uint8_t*>(span) + phase + kHashChars * threadIdx.x;
#pragma unroll
    for (uint32_t m = 0; m < kHashChars; ++m) s[m] = (uint8_t)(c[m >> 2] >> (8 * (m & 3)));
  }
  __syncthreads();
  // positions count from the aligned block that holds the span's first byte; only [phase, phase + len) is stored
  const uint32_t blocks = (phase + len + 15) / 16;
  for (uint32_t b = threadIdx.x; b < blocks; b += kEncBlock)
    b64d::put_block<false>(base - phase, 16 * b, phase, phase + len, span[b]);
}

// Whether the 27 bytes at s are the characters c: the aligned dwords that hold
// them, shifted into place.  The eighth dword holds a byte of the string only
// at phases 2 and 3.
__device__ __forceinline__ bool same_string(const uint8_t* s, const uint32_t c[7]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(s);
  const uint32_t sh = (uint32_t)(a & 3u);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(a - sh);
  uint32_t d[8];
#pragma unroll
  for (int k = 0; k < 7; ++k) d[k] = q[k];
  d[7] = sh >= 2 ? q[7] : 0u;
  uint32_t diff = 0;
#pragma unroll
  for (int j = 0; j < 6; ++j) diff |= __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh) ^ c[j];
  diff |= (__builtin_amdgcn_alignbyte(d[7], d[6], sh) ^ c[6]) & 0xFFFFFFu;
  return diff == 0;
}

// The lanes of this workgroup that hold `flag`: *before = those in lower lanes
// of the workgroup, the return value all of them.  wsum is kMapBlock / 64
// words of LDS.  Reached by the whole workgroup.
__device__ __forceinline__ uint32_t wg_count(bool flag, uint32_t* wsum, uint32_t* before) {
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t b = __ballot(flag);
  if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  uint32_t lower = (uint32_t)__popcll(b & ((1ull << lane) - 1)), all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kMapBlock / 64; ++w) {
    const uint32_t s = wsum[w];
    lower += w < wave ? s : 0u;
    all += s;
  }
  *before = lower;
  return all;
}

// blockIdx.x = group of kMapBlock chunks.
__global__ void __launch_bounds__(kMapBlock) hash_text_compare_kernel(HashTextVerify v) {
  __shared__ uint8_t alpha[64];
  __shared__ uint32_t wsum[kMapBlock / 64];
  b64d::fill_alphabet(alpha);
  __syncthreads();
  const uint32_t i = blockIdx.x * kMapBlock + threadIdx.x;
  bool bad = false;
  if (i < v.n) {
    uint32_t c[7];
    digest_chars(alpha, v.digests + 20ull * i, c);
    // Flood.cpp:270: chunk.m_hash.compare(test) == 0 -- the length first, then every character
    bool ok = (v.hash_len ? v.hash_len[i] : kHashChars) == kHashChars;
    if (ok) ok = same_string(v.hashes + (v.hash_off ? v.hash_off[i] : (uint64_t)kHashChars * i), c);
    v.chunkmap[i] = ok ? '1' : '0';
    bad = !ok;
  }
  if (!v.counts) return;  // no list asked for: the same in every lane
  uint32_t before;
  const uint32_t all = wg_count(bad, wsum, &before);
  if (threadIdx.x == 0) v.counts[blockIdx.x] = all;
}

// One workgroup: counts[0, blocks) to their exclusive prefix sums, the total to *total.
__global__ void __launch_bounds__(kScanWidth) hash_text_scan_kernel(uint32_t* counts, uint32_t blocks,
                                                                    uint32_t* total) {
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
  if (threadIdx.x == 0) *total = carry;
}

// blockIdx.x = group of kMapBlock chunks; counts[] holds the groups' bases.
__global__ void __launch_bounds__(kMapBlock) hash_text_scatter_kernel(HashTextVerify v) {
  __shared__ uint32_t wsum[kMapBlock / 64];
  const uint32_t i = blockIdx.x * kMapBlock + threadIdx.x;
  const bool bad = i < v.n && v.chunkmap[i] == '0';
  uint32_t before;
  wg_count(bad, wsum, &before);
  if (bad) v.missing[v.counts[blockIdx.x] + before] = i;
}

}  // namespace

int launch_hash_text_encode(const uint8_t* digests, uint8_t* hashes, const uint64_t* hash_off, uint32_t n,
                            hipStream_t stream) {
  if (n == 0) return LBF_OK;
  hipLaunchKernelGGL(hash_text_encode_kernel, dim3((n + kEncBlock - 1) / kEncBlock), dim3(kEncBlock), 0, stream,
                     digests, hashes, hash_off, n);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

int launch_hash_text_verify(const HashTextVerify& v, hipStream_t stream) {
  if (v.n == 0) return LBF_OK;
  const uint32_t blocks = (uint32_t)map_blocks(v.n);
  hipLaunchKernelGGL(hash_text_compare_kernel, dim3(blocks), dim3(kMapBlock), 0, stream, v);
  LBF_HIP_TRY(hipGetLastError());
  if (!v.missing) return LBF_OK;
  hipLaunchKernelGGL(hash_text_scan_kernel, dim3(1), dim3(kScanWidth), 0, stream, v.counts, blocks, v.missing_count);
  LBF_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(hash_text_scatter_kernel, dim3(blocks), dim3(kMapBlock), 0, stream, v);
  LBF_HIP_TRY(hipGetLastError());
  return LBF_OK;
}

}  // namespace htext
}  // namespace lbf

using lbf::fail;
namespace ht = lbf::htext;

extern "C" uint64_t lbf_verify_hashes_launch_work(uint64_t n) { return ht::work_bytes(n); }

extern "C" int lbf_sha1_hashes_launch(const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_sizes,
                                      uint64_t n, char* d_hashes, const uint64_t* d_hash_offsets, uint8_t* d_digests,
                                      uint8_t* d_work, void* stream) {
  const std::string who = "lbf_sha1_hashes_launch";
  if (n == 0) return LBF_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_hashes || !d_work) return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_work) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digests and work must be 4-byte aligned");
  const std::initializer_list<lbf::DevTable> tables = {
      {d_offsets, 8, n, "offsets", true},
      {d_sizes, 4, n, "sizes", true},
      {d_hash_offsets, 8, n, "hash_offsets", true},
      {d_hash_offsets ? nullptr : d_hashes, ht::kHashChars, n, "hashes", false},  // slots by offset are the caller's
      {d_digests, 20, n, "digests", false},
      {d_work, 1, ht::work_bytes(n), "work", false}};
  if (int rc = lbf::tables_aligned(who, tables)) return rc;
  if (int rc = lbf::tables_fit(who, tables)) return rc;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* const dig = d_digests ? d_digests : d_work;
  if (int rc = lbf_sha1_launch(d_data, d_offsets, d_sizes, n, dig, nullptr, nullptr, st)) return rc;
  return ht::launch_hash_text_encode(dig, reinterpret_cast<uint8_t*>(d_hashes), d_hash_offsets, (uint32_t)n, st);
}

extern "C" int lbf_verify_hashes_launch(const uint8_t* d_data, const uint64_t* d_offsets, const uint32_t* d_sizes,
                                        uint64_t n, const char* d_hashes, const uint64_t* d_hash_offsets,
                                        const uint32_t* d_hash_lens, char* d_chunkmap, uint32_t* d_missing,
                                        uint32_t* d_missing_count, uint8_t* d_digests, uint8_t* d_work, void* stream) {
  const std::string who = "lbf_verify_hashes_launch";
  if (n == 0) return LBF_OK;
  if (!d_data || !d_offsets || !d_sizes || !d_hashes || !d_chunkmap || !d_work)
    return fail(LBF_ERR_INVALID, who + ": null argument");
  if (n > 0x7FFFFFFFull) return fail(LBF_ERR_INVALID, who + ": n exceeds 2^31-1 per launch");
  if ((d_hash_offsets != nullptr) != (d_hash_lens != nullptr))
    return fail(LBF_ERR_INVALID, who + ": hash_offsets and hash_lens go together");
  if ((d_missing != nullptr) != (d_missing_count != nullptr))
    return fail(LBF_ERR_INVALID, who + ": missing and missing_count go together");
  if ((reinterpret_cast<uintptr_t>(d_digests) & 3u) || (reinterpret_cast<uintptr_t>(d_work) & 3u))
    return fail(LBF_ERR_INVALID, who + ": digests and work must be 4-byte aligned");
  const std::initializer_list<lbf::DevTable> tables = {
      {d_offsets, 8, n, "offsets", true},
      {d_sizes, 4, n, "sizes", true},
      {d_hash_offsets, 8, n, "hash_offsets", true},
      {d_hash_lens, 4, n, "hash_lens", true},
      {d_hash_offsets ? nullptr : d_hashes, ht::kHashChars, n, "hashes", false},  // strings by offset are the caller's
      {d_chunkmap, 1, n, "chunkmap", false},
      {d_missing, 4, n, "missing", true},
      {d_missing_count, 4, 1, "missing_count", true},
      {d_digests, 20, n, "digests", false},
      {d_work, 1, ht::work_bytes(n), "work", false}};
  if (int rc = lbf::tables_aligned(who, tables)) return rc;
  if (int rc = lbf::tables_fit(who, tables)) return rc;
  hipStream_t st = (hipStream_t)stream;
  uint8_t* const dig = d_digests ? d_digests : d_work;
  if (int rc = lbf_sha1_launch(d_data, d_offsets, d_sizes, n, dig, nullptr, nullptr, st)) return rc;
  const ht::HashTextVerify v{dig,
                             reinterpret_cast<const uint8_t*>(d_hashes),
                             d_hash_offsets,
                             d_hash_lens,
                             reinterpret_cast<uint8_t*>(d_chunkmap),
                             d_missing ? reinterpret_cast<uint32_t*>(d_work + ht::counts_at(n)) : nullptr,
                             d_missing,
                             d_missing_count,
                             (uint32_t)n};
  return ht::launch_hash_text_verify(v, st);
}
