// b64_encode_plan.hpp -- the arithmetic of lbf_b64_encode_update_batch: which
// calls are refused, which characters of its chunk's text a piece writes, where
// a launch's characters lie on the device (at their text position mod 16, so
// the kernel's 16-byte stores apply), and how they are copied back.  Pieces are
// cut into launches by update_plan.hpp's update_launches (an encoder state may
// be stopped at any byte, so its cuts at multiples of 64 do).  No HIP, no
// threads, no environment, no I/O: every rule here runs in a CPU test
// (tests/c/b64_encode_plan_tests.cpp).  b64_encode_batch.cpp drives the stream
// with it.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "b64_encode_update.hpp"
#include "b64_update_plan.hpp"
#include "lbf_hash.h"
#include "update_plan.hpp"

namespace lbf {

// Why a state pair cannot continue a chunk, or empty.
inline std::string b64_enc_state_fault(const lbf_b64_enc_state& e, const lbf_sha1_state& s) {
  if (e.layout > 1) return "layout " + std::to_string(e.layout) + " > 1";
  if (e.zero != 0) return "zero field is not zero";
  if (e.taken >= b64e::kEncMaxTaken) return "taken is 2^61 bytes or more";
  if (e.ncarry != e.taken % 3)
    return "ncarry " + std::to_string(e.ncarry) + " is not taken " + std::to_string(e.taken) + " % 3";
  if (e.carry >> (8 * e.ncarry)) return "carry holds more than ncarry bytes";
  if (s.buffered > 63 || s.buffered != s.total % 64)
    return "SHA state is corrupt (buffered " + std::to_string(s.buffered) + ", total " + std::to_string(s.total) + ")";
  if (s.total != e.taken)
    return "SHA state total " + std::to_string(s.total) + " is not taken " + std::to_string(e.taken);
  return std::string();
}

// The checks of one call, all before any GPU work.  Returns the first piece
// that is refused (and why), or kNoPiece.
inline uint64_t b64_encode_check(const lbf_b64_enc_state* enc, const lbf_sha1_state* sha, uint64_t n_states,
                                 const uint32_t* state_of, uint64_t data_len, const uint64_t* offsets,
                                 const uint32_t* sizes, uint64_t n, uint64_t text_len, const uint64_t* text_offsets,
                                 const uint32_t* text_caps, std::string& why) {
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t o = offsets[i], sz = sizes[i], cap = text_caps[i], to = text_offsets[i];
    if (o > data_len || sz > data_len - o) {
      why = "lies outside [data, data+data_len)";
      return i;
    }
    if (cap > b64e::kEncMaxTextCap) {
      why = "has a text slot of " + std::to_string(cap) + " characters, more than a chunk of 1 GiB has";
      return i;
    }
    if (to > text_len || cap > text_len - to) {
      why = "has its slot outside [text, text+text_len)";
      return i;
    }
    const uint64_t s = update_state_of(state_of, i);
    if (s >= n_states) {
      why = "names state " + std::to_string(s) + " of " + std::to_string(n_states);
      return i;
    }
    const std::string fault = b64_enc_state_fault(enc[s], sha[s]);
    if (!fault.empty()) {
      why = "continues a corrupt state: " + fault;
      return i;
    }
    if (enc[s].taken + sz > b64e::kEncMaxChunk) {
      why = "takes its chunk to " + std::to_string(enc[s].taken + sz) + " bytes, more than 1 GiB";
      return i;
    }
  }
  std::vector<uint64_t> idx(n);
  for (uint64_t i = 0; i < n; ++i) idx[i] = i;
  if (state_of) {  // two pieces of one state: the order they would be encoded in is undefined
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
    return text_offsets[a] != text_offsets[b] ? text_offsets[a] < text_offsets[b] : a < b;
  });
  uint64_t bad = kNoPiece, end = 0;
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t i = idx[k];
    if (text_caps[i] == 0) continue;
    if (text_offsets[i] < end) bad = std::min(bad, i);
    end = std::max(end, text_offsets[i] + text_caps[i]);
  }
  if (bad != kNoPiece) {
    why = "has a slot that overlaps another state's";
    return bad;
  }
  return kNoPiece;
}

// The characters of its chunk's text that a cut writes: positions [lo, hi),
// both clipped to the cap; `length` is the text length a final cut reports
// (the chunk's, or cap + 1 when it does not fit).
struct B64EncSpan {
  uint64_t lo = 0, hi = 0, length = 0;
};

inline B64EncSpan b64_encode_span(uint64_t taken, uint64_t size, bool final_piece, bool flat, uint64_t cap) {
  const uint64_t t1 = taken + size;
  const uint64_t p0 = b64e::group_pos(taken / 3, flat);
  const uint64_t p1 = b64e::group_pos(t1 / 3, flat) + (final_piece && t1 % 3 ? 4 : 0);
  return B64EncSpan{std::min(p0, cap), std::min(p1, cap), p1 <= cap ? p1 : cap + 1};
}

// Where one cut's characters lie on the device.
struct B64EncPlace {
  uint64_t dev = 0;   // device position of its first new character, = (text position) mod 16
  uint64_t room = 0;  // how many it writes there
  uint64_t slot = 0;  // the kernel's slot start: dev - text position, mod 2^64
};

// Areas follow one another, each moved up to its text position mod 16: the
// kernel's blocks are 16-byte blocks of the chunk's text, and whole ones are
// stored with 16-byte stores where the address allows.  Returns the area's size.
inline uint64_t b64_encode_places(const std::vector<B64EncSpan>& spans, std::vector<B64EncPlace>& places) {
  places.assign(spans.size(), B64EncPlace{});
  uint64_t cursor = 0;
  for (size_t k = 0; k < spans.size(); ++k) {
    B64EncPlace& p = places[k];
    p.room = spans[k].hi - spans[k].lo;
    p.dev = cursor + ((spans[k].lo - cursor) & 15u);
    p.slot = p.dev - spans[k].lo;  // mod 2^64: the kernel adds the text position back
    cursor = p.dev + p.room;
  }
  return cursor;
}

// Copy-back: cut k put size[k] characters at device position dev[k], which
// belong at host position host[k]; ranges that touch on both sides travel as
// one run (b64_update_plan.hpp's rule).
inline void b64_encode_copyback(const std::vector<uint64_t>& dev, const std::vector<uint64_t>& host,
                                const std::vector<uint32_t>& size, std::vector<Run>& runs) {
  b64_update_copyback(dev, host, size, runs);
}

}  // namespace lbf
