// b64_update_plan.hpp -- the arithmetic of lbf_b64_update_batch: which calls
// are refused, how many bytes a piece of text can decode to at most, where a
// launch's decoded bytes lie on the device (at their chain position mod 64, so
// the update kernel's aligned loop applies), and how they are copied back.
// Text is cut into launches by update_plan.hpp's update_launches (a base64
// state may be stopped at any character, so its cuts at multiples of 64 do).
// No HIP, no threads, no environment, no I/O: every rule here runs in a CPU
// test (tests/c/b64_update_plan_tests.cpp).  b64_update_batch.cpp drives the
// stream with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "lbf_hash.h"
#include "update_plan.hpp"

namespace lbf {

constexpr uint64_t kB64MaxChunk = 1ull << 30;  // the wire calls' bound on a chunk

// The bytes a state with `ncarry` pending sextets can gain from `len`
// characters: every complete group three, and a closing "xx=" / "xxx=" at most
// two more.
inline uint64_t b64_decode_bound(uint32_t ncarry, uint64_t len) { return 3 * ((ncarry + len) / 4) + 2; }

// Why a state pair cannot continue a chunk of `cap` bytes, or empty.
inline std::string b64_state_fault(const lbf_b64_state& b, const lbf_sha1_state& s, uint64_t cap) {
  if (b.ncarry > 3) return "ncarry " + std::to_string(b.ncarry) + " > 3";
  if (b.carry >> (6 * b.ncarry)) return "carry holds more than ncarry sextets";
  if (b.ended > 1) return "ended " + std::to_string(b.ended) + " > 1";
  if (b.zero != 0) return "zero field is not zero";
  if (!b.ended && b.decoded % 3 != 0) return "decoded " + std::to_string(b.decoded) + " is no multiple of 3 before '='";
  if (b.decoded >= kUpdateMaxTotal) return "decoded is 2^61 bytes or more";
  if (s.buffered > 63 || s.buffered != s.total % 64)
    return "SHA state is corrupt (buffered " + std::to_string(s.buffered) + ", total " + std::to_string(s.total) + ")";
  if (s.total != std::min<uint64_t>(b.decoded, cap))
    return "SHA state total " + std::to_string(s.total) + " is not min(decoded " + std::to_string(b.decoded) +
           ", chunk size " + std::to_string(cap) + ")";
  return std::string();
}

// The checks of one call, all before any GPU work.  Returns the first piece
// that is refused (and why), or kNoPiece.
inline uint64_t b64_update_check(const lbf_b64_state* b64, const lbf_sha1_state* sha, uint64_t n_states,
                                 const uint32_t* state_of, uint64_t text_len, const uint64_t* text_offsets,
                                 const uint32_t* text_lens, uint64_t n, const uint32_t* caps, uint64_t out_len,
                                 const uint64_t* out_offsets, std::string& why) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t o = text_offsets[i], l = text_lens[i], cap = caps[i], oo = out_offsets[i];
    if (o > text_len || l > text_len - o) {
      why = "has text outside [text, text+text_len)";
      return i;
    }
    if (cap > kB64MaxChunk) {
      why = "is of a chunk of " + std::to_string(cap) + " bytes, more than 1 GiB";
      return i;
    }
    if (oo > out_len || cap > out_len - oo) {
      why = "has its slot outside [out, out+out_len)";
      return i;
    }
    const uint64_t s = update_state_of(state_of, i);
    if (s >= n_states) {
      why = "names state " + std::to_string(s) + " of " + std::to_string(n_states);
      return i;
    }
    const std::string fault = b64_state_fault(b64[s], sha[s], cap);
    if (!fault.empty()) {
      why = "continues a corrupt state: " + fault;
      return i;
    }
  }
  std::vector<uint64_t> idx(n);
  for (uint64_t i = 0; i < n; ++i) idx[i] = i;
  if (state_of) {  // two pieces of one state: the order they would be decoded in is undefined
    std::sort(idx.begin(), idx.end(),
              [&](uint64_t a, uint64_t b) { return state_of[a] != state_of[b] ? state_of[a] < state_of[b] : a < b; });
    uint64_t bad = kNoPiece;
    for (uint64_t k = 1; k < n; ++k)
      if (state_of[idx[k]] == state_of[idx[k - 1]]) bad = std::min(bad, idx[k]);
    if (bad != kNoPiece) {
      why = "is the second piece of state " + std::to_string(state_of[bad]) + " in one call";
      return bad;
    }
  }
  // slots of different states may touch but not overlap (empty slots hold nothing)
  std::sort(idx.begin(), idx.end(), [&](uint64_t a, uint64_t b) {
    return out_offsets[a] != out_offsets[b] ? out_offsets[a] < out_offsets[b] : a < b;
  });
  uint64_t bad = kNoPiece, end = 0;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = idx[k];
    if (caps[i] == 0) continue;
    if (out_offsets[i] < end) bad = std::min(bad, i);
    end = std::max(end, out_offsets[i] + caps[i]);
  }
  if (bad != kNoPiece) {
    why = "has a slot that overlaps another state's";
    return bad;
  }
  return kNoPiece;
}

// Where one cut of text decodes to on the device.
struct B64Place {
  uint64_t dev = 0;   // device position of its first new byte, = (chain position) mod 64
  uint64_t room = 0;  // the most it can write there
  uint64_t slot = 0;  // the kernel's slot start: dev - chain position, mod 2^64
};

// Cut k continues a chain that has decoded `decoded[k]` bytes with ncarry[k]
// sextets pending into a chunk of cap[k] bytes, from len[k] characters.  The
// kernel writes chain positions [min(decoded, cap), cap) at most, so the room
// is the decode bound clipped to what is left of the slot; areas follow one
// another, each moved up to its chain position mod 64.  Returns the area's size.
inline uint64_t b64_update_places(const std::vector<uint64_t>& decoded, const std::vector<uint32_t>& ncarry,
                                  const std::vector<uint32_t>& len, const std::vector<uint32_t>& cap,
                                  std::vector<B64Place>& places) {
  places.assign(decoded.size(), B64Place{});
  uint64_t cursor = 0;
  for (size_t k = 0; k < decoded.size(); ++k) {
    const uint64_t at = std::min<uint64_t>(decoded[k], cap[k]);
    B64Place& p = places[k];
    p.room = std::min<uint64_t>(b64_decode_bound(ncarry[k] & 3u, len[k]), cap[k] - at);
    p.dev = cursor + ((at - cursor) & 63u);
    p.slot = p.dev - at;  // mod 2^64: the kernel adds the chain position back
    cursor = p.dev + p.room;
  }
  return cursor;
}

// Copy-back: piece k put size[k] bytes at device position dev[k], which belong
// at host position host[k].  Ranges that touch on both sides travel as one
// run (stage_plan.hpp's Run: src = device, dst = host).
inline void b64_update_copyback(const std::vector<uint64_t>& dev, const std::vector<uint64_t>& host,
                                const std::vector<uint32_t>& size, std::vector<Run>& runs) {
  runs.clear();
  for (size_t k = 0; k < dev.size(); ++k) {
    if (size[k] == 0) continue;
    if (!runs.empty() && runs.back().src + runs.back().len == dev[k] && runs.back().dst + runs.back().len == host[k]) {
      runs.back().len += size[k];
      continue;
    }
    runs.push_back(Run{dev[k], size[k], host[k], size[k], 0});
  }
}

}  // namespace lbf
